"""The workspaces of the point-cloud, registration, feature, TSDF, pose-graph and message entry points, as the caller sees them,
are what the parent of the carver refactor (csrc/gsr_carve.h) answered: tests/golden/workspace_layouts_parent.json holds every
size function over a grid of sizes (0, 1, the 256-byte rounding edges of 4-, 8- and 16-byte elements, 2^24 + 1, the largest sizes
accepted) and the return code and error text of every entry point called with a workspace one byte short and with none, recorded
from that commit's library by tools/record_workspace_layouts.py; the same calls against the built library must give the same
integers and the same strings.  None of it needs a GPU: the size functions and the early returns run on the host.

The carver itself, and the neighbour-search blob of csrc/knn_common.h described with it, are checked by a stand-alone program
(tests/workspace_carve_main.cpp) under AddressSanitizer and UBSan: sizing and viewing agree, spans aligned, ordered, disjoint, inside."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gaussian-splatting-slam_amd", "csrc")


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_workspace_layouts", os.path.join(ROOT, "tools", "record_workspace_layouts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "workspace_layouts_parent.json")) as f:
        return json.load(f)


def test_every_size_equals_the_parents_record(recorder, gold):
    from diff_gaussian_rasterization import _C
    got = recorder.record_sizes(_C.lib())
    assert sorted(got) == sorted(gold["sizes"])
    assert sum(len(v) for v in gold["sizes"].values()) == 863
    wrong = [(name, g, w) for name in gold["sizes"] for g, w in zip(got[name], gold["sizes"][name]) if list(g) != list(w)]
    assert all(len(got[name]) == len(gold["sizes"][name]) for name in got)
    assert not wrong, "%d sizes differ from the parent's (name, got, want), e.g. %s" % (len(wrong), wrong[:5])


def test_every_size_error_equals_the_parents_record(recorder, gold):
    from diff_gaussian_rasterization import _C
    got = recorder.record_errors(_C.lib())
    assert len(got) == len(gold["errors"]) == 162
    # every probe with a workspace one byte short ends at the size check, none at an argument check in front of it
    short = [e for e in gold["errors"] if e[2] == "short"]
    assert len(short) == 81 and all("needed" in e[4] or "too small" in e[4] for e in short)
    wrong = [(g, w) for g, w in zip(got, gold["errors"]) if list(g) != list(w)]
    assert not wrong, "%d return codes or messages differ from the parent's (got, want), e.g. %s" % (len(wrong), wrong[:3])


def test_carver_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"      # knn_common.h includes the HIP headers; host compiler only
    exe = str(tmp_path / "workspace_carve_main")
    # (the sanitizer runtimes linked into the program: it runs whatever else the process environment preloads)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__=1", "-I", CSRC, "-I", os.path.join(rocm, "include"),
                    os.path.join(HERE, "workspace_carve_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 100000]
    assert [ln for ln in lines if ln.startswith("nn ")] == [ln for ln in lines if ln.startswith("nn ") and ln.endswith(" ok")]
    assert [int(ln.split()[1][2:]) for ln in lines if ln.startswith("nn ")] == sizes
    assert [int(ln.split()[1][2:]) for ln in lines if ln.startswith("mixed ")] == sizes[1:]
