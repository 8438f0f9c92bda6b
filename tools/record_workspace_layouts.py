"""Records what the workspace-taking entry points outside the rasterizer answer on the host, for
tests/test_workspace_layouts_cpu.py: every size function over a grid of sizes, and the return code and gsr_last_error() text of
every entry point that reaches its size check before its first HIP call, once with a workspace one byte short and once with a
NULL workspace.  It only loads the built library and calls it (no GPU: nothing here gets past the checks).

    python tools/record_workspace_layouts.py            # writes tests/golden/workspace_layouts_parent.json

Run it on the commit whose behaviour is to be pinned; record(lib) is what the test replays against the library it finds.

Every workspace-taking entry point outside the rasterizer reaches its size check before its first HIP call, so every one is
probed; gsr_densify_apply reads the workspace gsr_densify_plan filled and is told no size, so it has no check to probe."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

BIG = (1 << 30) - 1          # the largest row count gsr_bad_size accepts
# 0, 1, the 256-byte rounding edges of 16-, 8- and 4-byte elements, page-ish sizes, a cloud, past 2^24, the limits
GRID = [-1, 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 100000, (1 << 24) + 1, BIG, (1 << 31) - 1]
CROSS = [0, 1, 63, 64, 65, 257, 4097, 100000]

ONE_ARG = ["gsr_densify_workspace_bytes", "gsr_knn_workspace_bytes", "gsr_knn_k_workspace_bytes", "gsr_voxel_workspace_bytes",
           "gsr_outlier_workspace_bytes", "gsr_nn_index_bytes", "gsr_nn_order_workspace_bytes", "gsr_icp_workspace_bytes",
           "gsr_normals_workspace_bytes", "gsr_color_gradient_workspace_bytes", "gsr_icp_colored_workspace_bytes",
           "gsr_information_workspace_bytes", "gsr_fpfh_workspace_bytes", "gsr_feature_nn_workspace_bytes",
           "gsr_pc2_decode_workspace_bytes", "gsr_tsdf_extract_workspace_bytes", "gsr_transform_workspace_bytes"]
# the largest value of each argument an entry point accepts
TWO_ARG = {"gsr_odometry_workspace_bytes": (32767, 32767), "gsr_depth_register_workspace_bytes": (32767, 32767),
           "gsr_unproject_workspace_bytes": (32767, 32767), "gsr_posegraph_topology_bytes": (BIG, BIG),
           "gsr_posegraph_workspace_bytes": (BIG, BIG), "gsr_ransac_workspace_bytes": (BIG, 1 << 20)}
EXTRA = {"gsr_tsdf_extract_workspace_bytes": [(1 << 19) - 1, 1 << 19, (1 << 19) + 1]}


def record_sizes(lib):
    out = {}
    for name in ONE_ARG:
        out[name] = [[[p], int(getattr(lib, name)(p))] for p in GRID + EXTRA.get(name, [])]
    for name, (amax, bmax) in TWO_ARG.items():
        f = getattr(lib, name)
        out[name] = [[[a, b], int(f(a, b))] for a in CROSS + [amax] for b in CROSS + [bmax]]
    return out


def record_errors(lib):
    """[entry point, sizes, which pointer is short or NULL, return code, message] per probe."""
    from diff_gaussian_rasterization import _C
    host = (C.c_char * 4096)()      # a real host buffer behind every pointer nothing reads before the size check
    buf = C.addressof(host)
    out = []

    def probe(name, sizes, need, call):
        f = getattr(lib, name)
        for what, ws, nbytes in (("short", buf, need - 1), ("null", None, need)):
            rc = int(f(*call(ws, nbytes)))
            out.append([name, list(sizes), what, rc, lib.gsr_last_error().decode("utf-8", "replace")])

    for P in (1, 65, 100000):
        probe("gsr_voxel_down_sample", [P], lib.gsr_voxel_workspace_bytes(P),
              lambda ws, n: (P, buf, None, 0.05, None, buf, None, None, 16, buf, ws, n, None))
        probe("gsr_statistical_outliers", [P], lib.gsr_outlier_workspace_bytes(P),
              lambda ws, n: (P, buf, 10, 2.0, buf, None, None, ws, n, None))
        probe("gsr_knn_dist2", [P], lib.gsr_knn_workspace_bytes(P), lambda ws, n: (P, buf, 0, buf, ws, n, None))
        probe("gsr_knn_k", [P], lib.gsr_knn_k_workspace_bytes(P), lambda ws, n: (P, buf, 3, buf, None, ws, n, None))
        probe("gsr_nn_index_build", [P], lib.gsr_nn_index_bytes(P), lambda ws, n: (P, buf, ws, n, None))
        probe("gsr_nn_query_order", [P], lib.gsr_nn_order_workspace_bytes(P),
              lambda ws, n: (100, buf, P, buf, buf, buf, ws, n, None))
        probe("gsr_icp_update", [P], lib.gsr_icp_workspace_bytes(P), lambda ws, n: (P, buf, 100, buf, buf, buf, buf, ws, n, None))
        probe("gsr_icp_update_plane", [P], lib.gsr_icp_workspace_bytes(P),
              lambda ws, n: (P, buf, 100, buf, buf, buf, buf, buf, ws, n, None))
        probe("gsr_icp_update_colored", [P], lib.gsr_icp_colored_workspace_bytes(P),
              lambda ws, n: (P, buf, buf, 100, buf, buf, buf, buf, buf, 0.5, buf, buf, ws, n, None))
        probe("gsr_estimate_normals", [P], lib.gsr_normals_workspace_bytes(P),
              lambda ws, n: (P, buf, 0.1, 10, None, buf, None, None, ws, n, None))
        probe("gsr_color_gradient", [P], lib.gsr_color_gradient_workspace_bytes(P),
              lambda ws, n: (P, buf, buf, buf, 0.1, 10, buf, None, None, ws, n, None))
        probe("gsr_registration_information", [P], lib.gsr_information_workspace_bytes(P),
              lambda ws, n: (100, buf, P, buf, buf, buf, ws, n, None))
        probe("gsr_compute_fpfh", [P], lib.gsr_fpfh_workspace_bytes(P),
              lambda ws, n: (P, buf, buf, 0.1, 10, buf, None, None, ws, n, None))
        probe("gsr_feature_nn", [P], lib.gsr_feature_nn_workspace_bytes(P),
              lambda ws, n: (P, buf, 100, buf, 33, buf, None, ws, n, None))
        counts = (C.c_int64 * 3)()
        probe("gsr_densify_plan", [P], lib.gsr_densify_workspace_bytes(P),
              lambda ws, n: (P, buf, buf, buf, buf, 0.0002, 0.005, 1.0, 0.01, 0, ws, n, counts, None))
        layout = _C.gsr_pc2_layout(P, 1, 16, 16 * P, 0, (C.c_int32 * 3)(0, 4, 8), (C.c_int32 * 3)(7, 7, 7), -1, 0)
        probe("gsr_pc2_decode", [P], lib.gsr_pc2_decode_workspace_bytes(P),
              lambda ws, n: (C.byref(layout), buf, 16 * P, None, -1e30, 1e30, 1, buf, None, None, 16, buf, ws, n, None))
    for K in (1, 65, 100000):
        probe("gsr_transform_gaussians", [K], lib.gsr_transform_workspace_bytes(K),
              lambda ws, n: (10, None, K, buf, ws, n, buf, buf, buf, None, 0, None, None))
    vol = _C.gsr_tsdf_volume((C.c_double * 3)(0.0, 0.0, 0.0), 0.01, 0.04, 3.0, 64.0, 0.0)
    for B in (1, 65, 1 << 19):
        need = lib.gsr_tsdf_extract_workspace_bytes(B)
        probe("gsr_tsdf_extract_points", [B], need,
              lambda ws, n: (C.byref(vol), B, buf, buf, buf, buf, buf, 1.0, 16, buf, buf, buf, buf, ws, n, None))
        probe("gsr_tsdf_extract_triangles", [B], need,
              lambda ws, n: (C.byref(vol), B, buf, buf, buf, buf, buf, 1.0, 16, buf, buf, buf, ws, n, None))
    Kd = (C.c_float * 4)(500.0, 500.0, 4.0, 4.0)
    T = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    Ko = (C.c_double * 4)(500.0, 500.0, 32.0, 24.0)
    for W, H in ((1, 1), (65, 3), (640, 480)):
        probe("gsr_depth_register", [W, H], lib.gsr_depth_register_workspace_bytes(W, H),
              lambda ws, n: (8, 8, buf, Kd, Kd, T, W, H, buf, buf, ws, n, None))
        probe("gsr_odometry_update", [W, H], lib.gsr_odometry_workspace_bytes(W, H),
              lambda ws, n: (W, H, Ko, buf, buf, buf, buf, buf, 0.5, 0.1, 1, buf, buf, ws, n, None))
        base = _C.gsr_unproject_params(H, W, 0.5, 0.5, buf, 1, 0.1, 10.0, 0.5, 0.05)
        pk = _C.gsr_unproject_params_k(base, 0.0, 0.0)
        need = lib.gsr_unproject_workspace_bytes(W, H)
        probe("gsr_unproject_rgbd", [W, H], need,
              lambda ws, n: (C.byref(base), buf, buf, None, None, buf, buf, 16, buf, ws, n, None))
        probe("gsr_unproject_rgbd_k", [W, H], need,
              lambda ws, n: (C.byref(pk), buf, buf, None, None, buf, buf, 16, buf, ws, n, None))
    for M, n_trials in ((1, 1), (65, 4097), (100000, 1 << 20)):
        probe("gsr_ransac_feature_matching", [M, n_trials], lib.gsr_ransac_workspace_bytes(M, n_trials),
              lambda ws, n: (100, buf, 100, buf, M, buf, 0.1, 3, 0.9, 0, 0, n_trials, buf, ws, n, None, None))
    for N, E in ((1, 0), (5, 4), (257, 300)):
        need = lib.gsr_posegraph_workspace_bytes(N, E)
        probe("gsr_posegraph_solve", [N, E], need, lambda ws, n: (N, E, buf, buf, buf, 1.0, 0.1, 10, buf, buf, ws, n, None))
        probe("gsr_posegraph_optimize", [N, E], need,
              lambda ws, n: (N, E, buf, buf, buf, buf, buf, 1.0, 10, 1e-6, 1e-6, 0.1, 10, buf, buf, buf, ws, n, None))
        edges = (C.c_int32 * (2 * max(E, 1)))(*[v for k in range(E) for v in (k % N, (k + 1 + k // N) % N)])
        fixed = (C.c_uint8 * N)(1)
        tneed = lib.gsr_posegraph_topology_bytes(N, E)
        scratch = (C.c_char * tneed)()
        probe("gsr_posegraph_topology", [N, E], tneed,
              lambda ws, n: (N, E, edges, fixed, C.addressof(scratch), ws, n, None))
    return out


def record(lib):
    return {"sizes": record_sizes(lib), "errors": record_errors(lib)}


def main():
    from diff_gaussian_rasterization import _C
    rec = record(_C.lib())
    path = os.path.join(ROOT, "tests", "golden", "workspace_layouts_parent.json")
    with open(path, "w") as f:      # one case per line
        f.write('{\n"sizes": {\n')
        f.write(",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(c) for c in v)) for k, v in rec["sizes"].items()))
        f.write('\n},\n"errors": [\n')
        f.write(",\n".join(json.dumps(e) for e in rec["errors"]))
        f.write("\n]\n}\n")
    print("%s: %d sizes, %d error probes" % (path, sum(len(v) for v in rec["sizes"].values()), len(rec["errors"])))


if __name__ == "__main__":
    main()
