"""csrc/densify.hip against tests/densify_reference.py, row by row: every split child against the float64 replay of its own draw
(the stream is counter based: seed, source row, copy * 3 + axis), every keep / clone / split decision against `plan` wherever the
reference calls it decided, non-finite parameters, and k_densify_stats against float64 with its derived bound.  The bounds are
max(2^-24, 4 x the float32 replay's own figure) from the reference alone; figures are printed before they are asserted."""
import functools

import numpy as np
import pytest
import torch

import densify_reference as DR
from scene_utils import GaussianModel, make_gaussians
from scene_utils.synthetic import RawGaussians

pytestmark = pytest.mark.gpu

ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
COPIED = ("f_dc", "f_rest", "opacity", "rotation")


def _t(a):
    return torch.from_numpy(np.array(a))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _densify(name, seed=None):
    """One densify_and_prune call on a case's rows -> counts, source rows, the new parameters and moments (numpy)"""
    c = DR.case(name)
    p = c["params"]
    raw = RawGaussians(_t(p["xyz"]), _t(p["f_dc"]), _t(p["f_rest"]), _t(p["scaling"]), _t(p["rotation"]), _t(p["opacity"]), c["deg"])
    model = GaussianModel.from_raw(raw.to("cuda"))
    opt = model.training_setup(optimizer="hip", percent_dense=c["percent_dense"])
    if c["moments"] is not None:
        for n, a in ATTRS.items():
            st = opt.state[getattr(model, a)]
            st["step"] = torch.tensor(1.0)
            st["exp_avg"], st["exp_avg_sq"] = _t(c["moments"][n][0]).cuda(), _t(c["moments"][n][1]).cuda()
    model.xyz_gradient_accum, model.denom, model.max_radii2D = _t(c["accum"]).cuda(), _t(c["denom"]).cuda(), _t(c["max_radii"]).cuda()
    seed = c["seed"] if seed is None else seed
    nk, nc, ns, src = model.densify_and_prune(c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], None, seed=seed,
                                              return_source=True)
    torch.cuda.synchronize()
    newP = nk + nc + 2 * ns
    out = {n: getattr(model, a).detach().cpu().numpy() for n, a in ATTRS.items()}
    assert all(v.shape[0] == newP for v in out.values()) and src.shape == (newP,)
    assert model.xyz_gradient_accum.shape == (newP, 1) and model.denom.shape == (newP, 1) and model.max_radii2D.shape == (newP,)
    assert float(model.xyz_gradient_accum.abs().sum() + model.denom.abs().sum() + model.max_radii2D.abs().sum()) == 0
    mom = None
    if c["moments"] is not None:
        mom = {}
        for n, a in ATTRS.items():
            st = opt.state[getattr(model, a)]
            mom[n] = (st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
    for g in opt.param_groups:
        assert g["params"][0] is getattr(model, ATTRS[g["name"]])
    return dict(nk=nk, nc=nc, ns=ns, src=src.cpu().numpy().astype(np.int64), params=out, moments=mom, seed=seed & 0xFFFFFFFF)


_run = functools.lru_cache(maxsize=None)(_densify)


def _segments(r):
    nk, nc, ns = r["nk"], r["nc"], r["ns"]
    return dict(keep=slice(0, nk), clone=slice(nk, nk + nc), child0=slice(nk + nc, nk + nc + ns), child1=slice(nk + nc + ns, nk + nc + 2 * ns))


def _check_rows(name, r, label=""):
    """Sections A of the issue on one run: copied values and moments bit for bit, zero moments of new rows, copy 1 exactly ns rows
    behind copy 0, every child position and scaling within its bound of the float64 replay.  -> the printed figures"""
    c = DR.case(name)
    seg, src = _segments(r), r["src"]
    for k in ("keep", "clone", "child0"):
        assert (np.diff(src[seg[k]]) > 0).all(), k                                 # row order within each group
    assert np.array_equal(src[seg["child0"]], src[seg["child1"]])
    new = slice(r["nk"], src.shape[0])
    for n in DR.NAMES:
        got = r["params"][n]
        for k in ("keep", "clone"):
            assert _same_bits(got[seg[k]], c["params"][n][src[seg[k]]]), (n, k)
        if n in COPIED:
            for k in ("child0", "child1"):
                assert _same_bits(got[seg[k]], c["params"][n][src[seg[k]]]), (n, k)
        if r["moments"] is not None:
            for j in range(2):
                assert _same_bits(r["moments"][n][j][seg["keep"]], c["moments"][n][j][src[seg["keep"]]]), (n, j)
                assert not _bits(r["moments"][n][j][new]).any(), (n, j)          # exact (positive) zeros
    ns = r["ns"]
    rows = src[seg["child0"]]
    ref = DR.children(c["params"], rows, r["seed"])
    got = (r["params"]["xyz"][r["nk"] + r["nc"]:].reshape(2, ns, 3), r["params"]["scaling"][r["nk"] + r["nc"]:].reshape(2, ns, 3))
    fig, B = DR.figures(got, ref), DR.bounds()
    print(f"densify_replay children {name}{label}: P {c['P']} keep {r['nk']} clone {r['nc']} split {ns}  "
          f"xyz {fig['xyz']:.3e} (bound {B['xyz']:.3e})  scaling {fig['scaling']:.3e} (bound {B['scaling']:.3e})")
    assert DR.within(got, ref) == (True, True), (name, fig)
    return fig


@pytest.mark.parametrize("name", DR.case_names())
def test_children_and_copied_rows(name):
    """A: every component of every child xyz within max(2^-24, 4 x YARDSTICK) S of the float64 replay, child scaling likewise
    relative to max(1, |value|); the other four parameters bit-equal to the source row; moments of new rows exact zeros; kept rows
    and clones bit for bit.  Each case has the rows it is there for."""
    c, r = DR.case(name), _run(name)
    assert r["nk"] >= c["expect"]["keep"] and r["nc"] >= c["expect"]["clone"] and r["ns"] >= c["expect"]["split"]
    if name == "all_split":
        assert (r["nk"], r["nc"], r["ns"]) == (0, 0, c["P"])
    if name == "all_clone":
        assert (r["nk"], r["nc"], r["ns"]) == (c["P"], c["P"], 0)
    if name == "none_selected":
        assert r["nc"] == 0 and r["ns"] == 0
    _check_rows(name, r)


@pytest.mark.parametrize("name", DR.case_names())
def test_decisions(name):
    """C: keep / clone / child of every row the reference calls decided (all constructed rows among them); undecided rows may go
    either way, there are at most 1 % of them."""
    c, r = DR.case(name), _run(name)
    p = DR.plan_of_case(c)
    flags = DR.flags_from_source(c["P"], r["nk"], r["nc"], r["ns"], r["src"])
    und = p["undecided"]
    wrong = {k: int((flags[k] != p[k][0])[~und].sum()) for k in ("keep", "clone", "child")}
    print(f"densify_replay decisions {name}: P {c['P']} undecided {int(und.sum())} wrong on decided rows {wrong}")
    assert int(und.sum()) <= DR.UNDECIDED_CAP * c["P"]
    if name.startswith("edges_"):
        assert not und[:len(DR.EDGE_ROWS)].any()
        ws = 1 if c["max_screen_size"] else 0
        for i, row in enumerate(DR.EDGE_ROWS):
            assert tuple(int(flags[k][i]) for k in ("keep", "clone", "child")) == DR.EDGE_EXPECT[i][ws], row[0]
    assert wrong == dict(keep=0, clone=0, child=0)


def test_seeds():
    """B: the same seed twice gives identical bits; seeds 0, 1, 0xFFFFFFFF and 2^32 + 5 (masked to 5 on the Python side) each match
    their replay; two seeds leave kept and cloned rows bit-identical and move every child."""
    a, b = _run("aniso"), _densify("aniso")
    assert (a["nk"], a["nc"], a["ns"]) == (b["nk"], b["nc"], b["ns"]) and np.array_equal(a["src"], b["src"])
    for n in DR.NAMES:
        assert _same_bits(a["params"][n], b["params"][n]), n
        for j in range(2):
            assert _same_bits(a["moments"][n][j], b["moments"][n][j]), n
    runs = {}
    for seed in (0, 1, 0xFFFFFFFF, (1 << 32) + 5):
        r = runs[seed] = _run("aniso", seed)
        assert r["seed"] == seed % (1 << 32)
        _check_rows("aniso", r, f" seed {seed}")
    r5 = _run("aniso", 5)
    assert _same_bits(runs[(1 << 32) + 5]["params"]["xyz"], r5["params"]["xyz"])
    seg = _segments(a)
    det = slice(0, a["nk"] + a["nc"])
    for r in list(runs.values()):
        assert np.array_equal(r["src"], a["src"])
        for n in DR.NAMES:
            assert _same_bits(r["params"][n][det], a["params"][n][det]), n
        ch = slice(seg["child0"].start, None)
        assert a["ns"] >= 500 and (_bits(r["params"]["xyz"][ch]) != _bits(a["params"]["xyz"][ch])).any(axis=1).all()
        assert _same_bits(r["params"]["scaling"][ch], a["params"]["scaling"][ch])
    x0, x1 = runs[0]["params"]["xyz"][seg["child0"].start:], runs[1]["params"]["xyz"][seg["child0"].start:]
    assert (_bits(x0) != _bits(x1)).any(axis=1).all()


def test_non_finite_parameters_leave_clean_rows_alone():
    """D: rows with NaN in one, two or three scaling axes and rows with NaN or +-inf opacity among clean rows.  Every clean row's
    output is bit-identical to the run where those rows are clean as well; the bad rows follow the reference (a NaN operand makes
    a comparison false: a NaN scaling axis keeps the row as it is, a NaN opacity is not low)."""
    c0, c1 = DR.case("nonfinite_clean"), DR.case("nonfinite")
    r0, r1 = _run("nonfinite_clean"), _run("nonfinite")
    bad = c1["bad_rows"]
    assert bad.shape[0] >= 100 and np.isnan(c1["params"]["scaling"][bad]).any(axis=1).sum() >= 70
    clean = np.ones(c1["P"], dtype=bool)
    clean[bad] = False
    for n in DR.NAMES:
        assert _same_bits(c0["params"][n][clean], c1["params"][n][clean])
    s0, s1 = _segments(r0), _segments(r1)
    for k in s0:
        m0, m1 = clean[r0["src"][s0[k]]], clean[r1["src"][s1[k]]]
        assert np.array_equal(r0["src"][s0[k]][m0], r1["src"][s1[k]][m1]), k
        for n in DR.NAMES:
            assert _same_bits(r0["params"][n][s0[k]][m0], r1["params"][n][s1[k]][m1]), (k, n)
            for j in range(2):
                assert _same_bits(r0["moments"][n][j][s0[k]][m0], r1["moments"][n][j][s1[k]][m1]), (k, n, j)
    p = DR.plan_of_case(c1)
    assert not p["undecided"][bad].any()
    flags = DR.flags_from_source(c1["P"], r1["nk"], r1["nc"], r1["ns"], r1["src"])
    got = np.stack([flags[k][bad] for k in ("keep", "clone", "child")], axis=1)
    want = np.stack([p[k][0][bad] for k in ("keep", "clone", "child")], axis=1)
    nan_axis = np.isnan(c1["params"]["scaling"][bad]).any(axis=1)
    print(f"densify_replay non-finite: bad rows {bad.shape[0]}, with a NaN scaling axis {int(nan_axis.sum())}, "
          f"decisions off the reference {int((got != want).any(axis=1).sum())} (on NaN-axis rows {int((got != want).any(axis=1)[nan_axis].sum())})")
    assert np.array_equal(want[nan_axis], np.tile([True, False, False], (int(nan_axis.sum()), 1)))      # kept as they are
    assert np.array_equal(got, want)
    assert np.isfinite(r1["params"]["xyz"]).all()                                                      # no NaN child was written


@pytest.mark.parametrize("P", [1, 256, 257, 5003])
def test_stats_kernel_against_float64(P):
    """E: k_densify_stats against float64 accum + hypot(gx, gy) with the bound u |accum + hypot| + (2 u + 3 u^2) hypot derived in
    densify_reference; denom and max_radii2D exact; rows with radii == 0 bit-untouched, NaN gradients included."""
    rng = np.random.default_rng(40 + P)
    f = np.float32
    g = (rng.standard_normal((P, 3)) * 10.0 ** rng.uniform(-3, 3, (P, 1))).astype(f)
    acc = (rng.random((P, 1)) * 10.0 ** rng.uniform(-4, 2, (P, 1))).astype(f)
    den = rng.integers(0, 5, (P, 1)).astype(f)
    mr = (rng.random(P) * 30).astype(f)
    radii = rng.integers(1, 60, P).astype(np.int32)
    radii[rng.random(P) < 0.4] = 0
    if P == 1:
        radii[0] = 7
    hidden = np.nonzero(radii == 0)[0]
    g[hidden[::2]] = np.nan
    g[hidden[1::4], 1] = np.inf
    m = GaussianModel.from_raw(make_gaussians(P, 0, seed=1).to("cuda"))
    m.training_setup(optimizer="hip")
    m.xyz_gradient_accum, m.denom, m.max_radii2D = _t(acc).cuda(), _t(den).cuda(), _t(mr).cuda()
    vsp = torch.zeros(P, 3, device="cuda", requires_grad=True)
    vsp.grad = _t(g).cuda()
    tr = _t(radii).cuda()
    m.add_densification_stats(vsp, tr > 0, tr)
    torch.cuda.synchronize()
    a, d, mx, bound = DR.stats(acc, den, mr, g, radii)
    ga, gd, gm = m.xyz_gradient_accum.cpu().numpy(), m.denom.cpu().numpy(), m.max_radii2D.cpu().numpy()
    vis = radii > 0
    assert vis.sum() >= min(P, 100) and (P == 1 or (hidden.shape[0] >= 50 and np.isnan(g[hidden]).any()))
    err = np.abs(ga.reshape(-1).astype(np.float64) - a)
    print(f"densify_replay stats P {P}: visible {int(vis.sum())}  largest |error| / bound {float((err[vis] / bound[vis]).max()):.3f}")
    assert (err[vis] <= bound[vis]).all()
    assert np.array_equal(gd.reshape(-1).astype(np.float64), d) and np.array_equal(gm.astype(np.float64), mx)
    assert _same_bits(ga[~vis], acc[~vis]) and _same_bits(gd[~vis], den[~vis]) and _same_bits(gm[~vis], mr[~vis])
