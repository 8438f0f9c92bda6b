"""tests/densify_reference.py on its own (no GPU): the float32 replay's figures - from which the bounds of
tests/test_densify_replay_gpu.py are derived - are the constants it stores; the normal stream is held to sampling bounds; no two
draws of one call share a counter for any map this project can hold; decisions and children agree with oracle/densify_oracle.py;
a transposed rotation is far outside the children's bound."""
import functools
import math

import numpy as np
import pytest
import torch

import densify_reference as DR
from oracle import densify_oracle as DO

N_STREAM = 1 << 21
SEED = 11


# ---------------------------------------------------------------------------------------------------------------------------------
# yardstick
# ---------------------------------------------------------------------------------------------------------------------------------
def test_yardstick_constants():
    """Recomputed over all cases, the float32 replay's largest figures ARE the constants (to their printed digits), the bounds are
    max(2^-24, 4 x), and every case that is there for its children has them."""
    worst = DR.yardstick_all()
    assert set(worst) == set(DR.YARDSTICK)
    for k, (v, _) in worst.items():
        assert abs(v - DR.YARDSTICK[k]) <= 1e-3 * DR.YARDSTICK[k], (k, v, DR.YARDSTICK[k])
        assert DR.bounds()[k] == max(2.0 ** -24, 4.0 * DR.YARDSTICK[k])
    for name in DR.case_names():
        assert DR.yardstick(name)[1] >= DR.case(name)["expect"]["split"], name


def test_a_transposed_rotation_is_outside_the_bound():
    """What the population statistics of tests/test_densify_gpu.py cannot see: children built with R^T miss the float64 children by
    the order of S itself, the float32 replay stays inside the bound."""
    c = DR.case("aniso")
    rows = DR.child_rows(c)
    ref = DR.children(c["params"], rows, c["seed"])
    assert DR.within(DR.children(c["params"], rows, c["seed"], np.float32), ref) == (True, True)
    wrong = DR.children(c["params"], rows, c["seed"], transpose_R=True)
    assert DR.within(wrong, ref)[0] is False
    assert DR.figures(wrong, ref)["xyz"] > 1e4 * DR.bounds()["xyz"]
    # ... and so are the two copies swapped (streams permuted) and another seed
    perm = dict(ref, xyz=ref["xyz"][::-1])
    assert DR.within(perm, ref)[0] is False
    assert DR.within(DR.children(c["params"], rows, c["seed"] + 1), ref)[0] is False


@pytest.mark.parametrize("name", DR.case_names())
def test_undecided_cap(name):
    """From the reference alone: at most 1 % of a case's rows are undecided, the constructed rows none."""
    c = DR.case(name)
    p = DR.plan_of_case(c)
    assert int(p["undecided"].sum()) <= DR.UNDECIDED_CAP * c["P"], (name, int(p["undecided"].sum()))
    dec = ~p["undecided"]
    for k, need in (("keep", c["expect"]["keep"]), ("clone", c["expect"]["clone"]), ("child", c["expect"]["split"])):
        assert int((p[k][0] & dec).sum()) >= need, (name, k)
    if name.startswith("edges_"):
        ws = 1 if c["max_screen_size"] else 0
        for i, row in enumerate(DR.EDGE_ROWS):
            assert not p["undecided"][i], row[0]
            assert tuple(int(p[k][0][i]) for k in ("keep", "clone", "child")) == DR.EDGE_EXPECT[i][ws], row[0]
    if "bad_rows" in c:
        assert not p["undecided"][c["bad_rows"]].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _streams(seed=SEED):
    idx = np.arange(N_STREAM)
    z = np.stack([DR.normals(seed, idx, s)[0] for s in range(6)])
    z.setflags(write=False)
    return z


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


def test_stream_uniform_integers():
    """u1 is never 0, u2 never 1; |z| <= sqrt(-2 ln 2^-24) = 5.768 in either arithmetic"""
    idx = np.arange(N_STREAM)
    for s in range(6):
        i1, i2 = DR.counter_uniforms(SEED, idx, s)
        assert i1.min() >= 1 and i1.max() <= 1 << 24 and i2.min() >= 0 and i2.max() < 1 << 24
    zmax = math.sqrt(-2.0 * math.log(2.0 ** -24))
    assert abs(zmax - 5.768) < 1e-3
    assert np.abs(_streams()).max() <= zmax
    z32 = DR.normals(SEED, idx[:1 << 16], 0, np.float32)[0]
    assert z32.dtype == np.float32 and np.abs(z32).max() <= np.float32(zmax)
    assert np.abs(z32 - _streams()[0, :1 << 16]).max() <= 4 * 2.0 ** -24 * zmax
    # the seed is masked to 32 bits, as the Python side of densify_and_prune does
    assert np.array_equal(DR.normals((1 << 32) + 5, idx[:64], 2)[0], DR.normals(5, idx[:64], 2)[0])


def test_stream_moments():
    """Per stream: |mean| <= 5 / sqrt(n) (5 standard errors of the mean of n unit normals), |std - 1| <= 5 / sqrt(2 n) (5 standard
    errors of a normal sample's standard deviation)."""
    z, n = _streams(), N_STREAM
    for s in range(6):
        assert abs(float(z[s].mean())) <= 5.0 / math.sqrt(n), s
        assert abs(float(z[s].std()) - 1.0) <= 5.0 / math.sqrt(2 * n), s


def test_stream_correlations():
    """Sample correlation of two independent normal samples of length n has standard deviation 1 / sqrt(n); every one of the 15
    pairs of streams (axes and copies), the lag-1 pairs along the index and the pairs of consecutive seeds (the trainer calls with
    seed + it) stay within 5 / sqrt(n)."""
    z, n = _streams(), N_STREAM
    lim = 5.0 / math.sqrt(n)
    worst = 0.0
    for a in range(6):
        for b in range(a + 1, 6):
            worst = max(worst, abs(_corr(z[a], z[b])))
    assert worst <= lim, worst
    for s in range(6):
        assert abs(_corr(z[s][:-1], z[s][1:])) <= lim, s
    z1 = _streams(SEED + 1)
    for s in range(6):
        assert abs(_corr(z[s], z1[s])) <= lim, s
    assert abs(_corr(z[0], z1[1])) <= lim and abs(_corr(z[1][:-1], z1[0][1:])) <= lim


def test_stream_kolmogorov_smirnov():
    """Distance of every stream's empirical distribution to N(0, 1) below the 1 % critical value 1.6276 / sqrt(n)"""
    z, n = _streams(), N_STREAM
    crit = 1.6276 / math.sqrt(n)
    k = np.arange(1, n + 1) / n
    for s in range(6):
        x = np.sort(z[s])
        cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())
        d = max(float((k - cdf).max()), float((cdf - (k - 1.0 / n)).max()))
        assert d <= crit, (s, d, crit)


def test_stream_counters_do_not_collide_within_a_map():
    """The inner counter is idx * A + stream * B (mod 2^32), A odd: two draws (i, s), (j, t) of one call share it exactly when
    i - j = (t - s) * B * A^-1 (mod 2^32).  For every stream difference 1..5 that index distance is beyond 2^28 rows - more rows than
    the 31-bit row count times 18 tensors could hold in memory; the smallest is 390 925 038 at difference 2."""
    a_inv = pow(DR.HASH_A, -1, 1 << 32)
    assert DR.HASH_A * a_inv % (1 << 32) == 1
    dist = {}
    for d in range(1, 6):
        x = d * DR.HASH_B * a_inv % (1 << 32)
        dist[d] = min(x, (1 << 32) - x)
        # the reference's own uint32 counter agrees: rows `dist` apart, streams d apart
        i, j = ((0, x) if x < (1 << 31) else ((1 << 32) - x, 0))
        assert DR.counter_of(i, d)[0] == DR.counter_of(j, 0)[0]
        assert dist[d] > 1 << 28, (d, dist[d])
    assert min(dist.values()) == dist[2] == 390_925_038
    idx = np.arange(1 << 16)
    c = np.concatenate([DR.counter_of(idx, s) for s in range(6)])
    assert np.unique(c).shape[0] == c.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle agreement
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle(c, normal_samples=None):
    t = lambda x: torch.from_numpy(np.array(x))                             # noqa: E731
    params = {n: t(c["params"][n]) for n in DR.NAMES}
    moments = {n: (None if c["moments"] is None else (t(c["moments"][n][0]), t(c["moments"][n][1]))) for n in DR.NAMES}
    return DO.densify_and_prune(params, moments, t(c["accum"]), t(c["denom"]), t(c["max_radii"]), c["max_grad"], c["min_opacity"],
                                c["extent"], c["max_screen_size"], c["percent_dense"], normal_samples=normal_samples)


@pytest.mark.parametrize("name", DR.case_names())
def test_plan_and_children_agree_with_the_oracle(name):
    """`plan` gives the oracle's keep / clone / child on every decided row; the oracle, fed the float64 normals of the rows IT
    selects, reproduces `children(float64)` within the children's bound (its own arithmetic is float32) and the scalings likewise."""
    c = DR.case(name)
    P = c["P"]
    p = DR.plan_of_case(c)
    # the rows the oracle splits (scene/gaussian_model.py:369-373), before it prunes: that many samples, copy-major
    with torch.no_grad():
        g = torch.from_numpy(np.array(c["accum"])) / torch.from_numpy(np.array(c["denom"]))
        g[g.isnan()] = 0.0
        sel = (g.squeeze(-1) >= c["max_grad"]) & (torch.exp(torch.from_numpy(np.array(c["params"]["scaling"]))).max(dim=1).values
                                                  > c["percent_dense"] * c["extent"])
    sel_rows = np.nonzero(sel.numpy())[0]
    z = np.concatenate([np.stack([DR.normals(c["seed"], sel_rows, cp * 3 + a)[0] for a in range(3)], axis=1) for cp in range(2)])
    ref_p, ref_m, info = _oracle(c, torch.from_numpy(z).float())
    src, kind = info["source"].numpy(), info["kind"].numpy()
    nk, nc, n2 = int((kind == 0).sum()), int((kind == 1).sum()), int((kind == 2).sum())
    assert n2 % 2 == 0 and np.array_equal(kind, np.repeat([0, 1, 2], [nk, nc, n2]))
    ns = n2 // 2
    flags = DR.flags_from_source(P, nk, nc, ns, src)
    dec = ~p["undecided"]
    for k in ("keep", "clone", "child"):
        assert np.array_equal(flags[k][dec], p[k][0][dec]), (name, k)
    rows = src[nk + nc:nk + nc + ns]
    assert np.array_equal(rows, src[nk + nc + ns:])
    assert ns >= c["expect"]["split"]
    ref = DR.children(c["params"], rows, c["seed"])
    got = (ref_p["xyz"].numpy()[nk + nc:].reshape(2, ns, 3), ref_p["scaling"].numpy()[nk + nc:].reshape(2, ns, 3))
    assert DR.within(got, ref) == (True, True), (name, DR.figures(got, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stats_bound_holds_for_the_float32_replay():
    """The derived bound of k_densify_stats, against plain float32 numpy (two products, an add, a square root, an add)"""
    rng = np.random.default_rng(3)
    f = np.float32
    P = 20000
    g = (rng.standard_normal((P, 3)) * 10.0 ** rng.uniform(-3, 3, (P, 1))).astype(f)
    acc = (rng.random(P) * 10.0 ** rng.uniform(-4, 2, P)).astype(f)
    radii = rng.integers(0, 3, P).astype(np.int32)
    a, d, m, bound = DR.stats(acc, np.zeros(P, f), np.zeros(P, f), g, radii)
    got = np.where(radii > 0, acc + np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]), acc)
    assert got.dtype == f and (np.abs(got.astype(np.float64) - a) <= bound).all()
    assert (bound[radii == 0] == 0).all() and (bound[radii > 0] <= 4 * 2.0 ** -24 * np.abs(a[radii > 0])).all()
