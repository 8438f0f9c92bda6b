"""tests/projection_reference.py on its own (no GPU): its float64 forward is the oracle's preprocess, its float64 backward is the
central finite difference of its forward and contracts with the oracle's per-pixel autograd, the float32 replay's figures - from
which the bounds of tests/test_projection_replay_gpu.py are derived - are the constants it imports, and no case has more than
2 % of its visible Gaussians undecided on any discrete value."""
import functools

import numpy as np
import pytest
import torch

import compositing_reference as CR
import projection_reference as PR

COLS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]          # the record values the backward carries a cotangent for
FD_EPS, FD_TOL = 1e-6, 1e-3                    # as tests/test_oracle_golden.py: step 1e-6, |fd - an| <= 1e-3 max(1, |an|)
FD_CASES = [("edge", f) for f in PR.FORMS] + [("needles", "base"), ("needles", "raw-aa-mod2.3"), ("tail_257", "cov-aa")]
ORACLE_CASES = [("edge", f) for f in PR.FORMS] + [(n, "base") for n in PR.case_names() if n != "edge"] + [("needles", "raw-aa-mod2.3")]


def _oracle_pre(inp, grad=False):
    """oracle.gs_oracle.preprocess on the float32 call arguments promoted to float64 (raw parameters activated in float64 first)"""
    from oracle import gs_oracle as O
    t = lambda x: None if x is None else torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(grad)
    leaves = dict(means3D=t(inp["means3D"]), opacities=t(inp["opacities"]), scales=t(inp["scales"]), rotations=t(inp["rotations"]),
                  cov3D=t(inp["cov3D"]), shs=t(inp["shs"]), colors=t(inp["colors"]),
                  means2D=torch.zeros(inp["means3D"].shape[0], 3, dtype=torch.float64, requires_grad=grad))
    op, sc, ro = leaves["opacities"], leaves["scales"], leaves["rotations"]
    if inp["raw"]:
        op, sc = torch.sigmoid(op), torch.exp(sc)
        ro = ro / torch.clamp_min(ro.norm(dim=1, keepdim=True), 1e-12)
    f64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    s = O.OracleSettings(int(inp["H"]), int(inp["W"]), float(inp["tanfovx"]), float(inp["tanfovy"]), torch.zeros(3, dtype=torch.float64),
                         float(inp["scale_modifier"]), f64(inp["viewmatrix"]).view(4, 4), f64(inp["projmatrix"]).view(4, 4),
                         int(inp["deg"]), f64(inp["campos"]), False, False, bool(inp["antialiasing"]))
    pre = O.preprocess(leaves["means3D"], leaves["means2D"], op, s, shs=leaves["shs"], colors_precomp=leaves["colors"],
                       scales=sc if leaves["cov3D"] is None else None, rotations=ro if leaves["cov3D"] is None else None,
                       cov3D_precomp=leaves["cov3D"])
    return pre, leaves, s


@pytest.mark.parametrize("name,form", ORACLE_CASES)
def test_forward_is_the_oracle(name, form):
    """Published constants, float64: means2D, conic, opacity, colours and depth to 1e-12 of their S (at least 1e-12 absolute); radii
    and the 3-sigma rectangle exactly wherever the reference calls them decided.  No published guard makes the two differ: the
    oracle has the same + 1e-7 on hom.w, the same 0.1 and 0.000025 floors; the + 1e-7 of 1 / (det^2 + 1e-7) is backward only."""
    inp = PR.case_inputs(name, form)
    ref = PR.forward(inp, np.float64, published=True)
    with torch.no_grad():
        pre, _, _ = _oracle_pre(inp)
    und = PR.undecided(ref)
    vis_o = pre.radii.numpy() > 0
    sure = ~und["visible"] & ~und["radius"] & ~und["rect"]
    assert np.array_equal(vis_o[sure], ref["visible_nat"][sure])
    v = vis_o & ref["visible_nat"]
    assert v.sum() >= min(1, inp["means3D"].shape[0] - 1)

    def close(got, want, S):
        return (np.abs(got - want)[v] <= 1e-12 * np.maximum(1.0, S[v])).all()
    assert close(ref["rec"][:, 0:2], pre.xy.numpy(), ref["S"][:, 0:2])
    assert close(ref["conic"], pre.conic.numpy(), ref["S_conic"])
    assert close(ref["rec"][:, 5], pre.opacity.numpy(), ref["S"][:, 5])
    assert close(ref["rec"][:, 7:10], pre.rgb.numpy(), ref["S"][:, 7:10])
    assert close(ref["rec"][:, 11], pre.depths.numpy(), ref["S"][:, 11])
    if inp["colors"] is None:
        assert np.array_equal((ref["rgb_pre"] < 0)[v], pre.clamped.numpy()[v])
    d = v & sure
    assert np.array_equal(ref["radius_nat"][d].astype(np.int64), pre.radii.numpy()[d])
    assert np.array_equal(ref["rect_nat"][d][:, :2], pre.rect_min.numpy()[d]) and np.array_equal(ref["rect_nat"][d][:, 2:], pre.rect_max.numpy()[d])
    # the scaled record words are the conic and the cut-off in base 2 (include/gsr.h "Projection rules")
    l2 = PR.LOG2E
    assert np.allclose(ref["rec"][v][:, 2:5], np.stack([-0.5 * l2 * ref["conic"][v][:, 0], -l2 * ref["conic"][v][:, 1], -0.5 * l2 * ref["conic"][v][:, 2]], 1), rtol=1e-14)
    op = ref["rec"][v][:, 5]
    with np.errstate(all="ignore"):
        assert np.allclose(ref["rec"][v][:, 6], np.where(op > 0, l2 * (-np.log(255.0 * op) - 0.01), l2), rtol=1e-13)


def _fd_inputs(inp):
    return [k for k in ("means3D", "opacities", "scales", "rotations", "cov3D", "shs", "colors") if inp.get(k) is not None]


@pytest.mark.parametrize("name,form", FD_CASES)
def test_backward_is_the_finite_difference_of_the_forward(name, form):
    """A random cotangent on the ten record values with a gradient path -> the ten sums -> the float64 backward, against central
    differences of the float64 forward (clamped t.x / t.y held constant, as the published backward treats them), every input
    coordinate of every surely visible Gaussian.  Step and tolerance as tests/test_oracle_golden.py.  The + 1e-7 of
    1 / (det^2 + 1e-7) is not in the forward: the check runs without it, and its effect is bounded by 1e-7 / det^2 of S."""
    inp = PR.case_inputs(name, form)
    ref = PR.forward(inp, np.float64)
    P = inp["means3D"].shape[0]
    und = PR.undecided(ref)
    rows = PR.continuous_ok(ref) & ~und["clamp"] & np.isfinite(ref["rec"]).all(axis=1) & (ref["rec"][:, 5] > 0)
    if inp["raw"]:
        rows &= np.isfinite(inp["opacities"])
    cot = np.random.default_rng(11).standard_normal((P, 10))
    sums = PR.sums_for_cotangent(inp, cot, published=False)
    cb = ref["rgb_pre"] < 0
    an = PR.backward(inp, sums, None, cb, rows, np.float64, guard_det2=False)
    on = PR.backward(inp, sums, None, cb, rows, np.float64, guard_det2=True)
    g = ref["g"]
    freeze = (g["tx"].v, g["ty"].v)
    det = g["det"].v
    for k in an["grads"]:
        assert (np.abs(on["grads"][k] - an["grads"][k])[rows] <= (1.0001e-7 / (det[rows, None] ** 2) + 1e-14) * an["S"][k][rows]).all(), k   # (+ the float64 rounding of the two results)
    assert np.abs(an["grads"]["means2D"][rows] - 0.5 * np.array([inp["W"], inp["H"]]) * cot[rows, :2]).max() <= 1e-9 * np.abs(cot).max() * inp["W"]

    def loss(x):
        f = PR.forward(x, np.float64, freeze=freeze)
        return (cot * f["rec"][:, COLS]).sum(axis=1)
    worst = 0.0
    for key in _fd_inputs(inp):
        base = np.asarray(inp[key], dtype=np.float64)
        flat = base.reshape(P, -1)
        gk = an["grads"][key].reshape(P, -1)
        for j in range(flat.shape[1]):
            if key == "shs" and j >= 3 * (inp["deg"] + 1) ** 2:
                assert not gk[:, j].any()
                continue
            eps = FD_EPS * np.maximum(1.0, np.abs(flat[:, j]))
            steps = [eps]
            if key == "cov3D":
                # entries from e^-8 to e^8, and a needle's det = a c - b^2 keeps five digits of them: the step is relative to the
                # entry (at least to a thousandth of the row's largest); a needle needs a hundredth of that (1e-2: -9.09, 1e-4:
                # -6.2369, 1e-6 .. 1e-8: -6.23667 on the e^-4 : 1 : e^4 one), where a small near splat is already in the rounding
                # of the loss, and an off-diagonal entry of 1e-10 beside 1e-2 wants the row's scale: any of four steps may agree
                e1 = FD_EPS * np.maximum(np.abs(flat[:, j]), 1e-3 * np.abs(flat).max(axis=1))
                steps = [FD_EPS * np.abs(flat).max(axis=1), e1, 1e-1 * e1, 1e-2 * e1]
            err = np.full(P, np.inf)
            for eps in steps:
                hi, lo = flat.copy(), flat.copy()
                with np.errstate(invalid="ignore"):
                    hi[:, j] += eps
                    lo[:, j] -= eps
                fd = (loss({**inp, key: hi.reshape(base.shape)}) - loss({**inp, key: lo.reshape(base.shape)})) / (2.0 * eps)
                with np.errstate(invalid="ignore"):
                    err = np.fmin(err, np.abs(fd - gk[:, j]) / np.maximum(1.0, np.abs(gk[:, j])))
            # a coordinate whose step crosses a switch (the AA floor, a colour at 0, the clamp) is not differentiable there
            hi = flat.copy()
            with np.errstate(invalid="ignore"):
                hi[:, j] += steps[0]                                                 # (the largest of the steps tried)
            f0, fh = PR.forward(inp, np.float64), PR.forward({**inp, key: hi.reshape(base.shape)}, np.float64)
            crossed = ((f0["in_x_nat"] != fh["in_x_nat"]) | (f0["in_y_nat"] != fh["in_y_nat"]) | (f0["aa_free_nat"] != fh["aa_free_nat"])
                       | ((f0["rgb_pre"] < 0) != (fh["rgb_pre"] < 0)).any(axis=1))
            if key == "rotations" and inp["raw"]:                                # ... nor is normalize where |q| crosses its 1e-12
                crossed |= (np.linalg.norm(flat, axis=1) > 1e-12) != (np.linalg.norm(hi, axis=1) > 1e-12)
            if key == "cov3D":
                # a splat far below a pixel (|cov2D| < 1 % of the 0.3 dilation): no step is both above the rounding of the loss and
                # below the curvature of sqrt(det0 / det) there; the same rows are differentiated through their scales in the other forms
                crossed |= np.maximum(g["a0"].v, g["c0"].v) < 3e-3
            ok = rows & ~crossed & np.isfinite(fd)
            worst = max(worst, float(err[ok].max(initial=0.0)))
            assert (err[ok] <= FD_TOL).all(), (key, j, int(np.argmax(np.where(ok, err, 0))), float(err[ok].max()))
    print(f"\n[FD] {name} / {form}: largest |fd - backward| / max(1, |backward|) = {worst:.2e} over {int(rows.sum())} Gaussians")


def test_backward_contracts_with_the_oracle_autograd():
    """One small scene through the oracle's compositing with autograd: its dL/d(inputs) are the reference backward of its own
    dL/d(record) (to 1e-9 of each tensor's largest magnitude) - the hand derivation and autograd agree, AA on."""
    from oracle import gs_oracle as O
    name = "single_tile"
    inp = PR.case_inputs(name, "aa")
    W, H = inp["W"], inp["H"]
    pre, leaves, s = _oracle_pre(inp, grad=True)
    for x in (pre.xy, pre.conic, pre.opacity, pre.rgb, pre.depths):
        x.retain_grad()
    point_list, ranges, _ = O.bin_instances(pre, W, H)
    s = s._replace(bg=torch.tensor([0.4, 0.25, 0.6], dtype=torch.float64))
    color, invd, _, _ = O.composite(pre, point_list, ranges, s.bg, W, H)
    gp, gd, _ = CR.upstream(W, H)
    ((color * torch.from_numpy(gp).double()).sum() + (invd[0] * torch.from_numpy(gd).double()).sum()).backward()
    z = pre.depths.detach().numpy()
    vis = pre.tiles_touched.numpy() > 0
    gz = np.zeros_like(z) if pre.depths.grad is None else pre.depths.grad.numpy()
    l2 = PR.LOG2E
    cg = pre.conic.grad.numpy()
    cot = np.concatenate([pre.xy.grad.numpy(), cg[:, :1] / (-0.5 * l2), cg[:, 1:2] / (-l2), cg[:, 2:] / (-0.5 * l2),
                          pre.opacity.grad.numpy()[:, None], pre.rgb.grad.numpy(), (-gz * z * z)[:, None]], axis=1)
    cot = np.where(vis[:, None], cot, 0.0)
    sums = PR.sums_for_cotangent(inp, cot, published=True)
    b = PR.backward(inp, sums, None, pre.clamped.numpy(), vis, np.float64, published=True, guard_det2=False)
    pairs = dict(means3D=leaves["means3D"], opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"],
                 shs=leaves["shs"])
    assert vis.sum() > 100
    for k, leaf in pairs.items():
        want = leaf.grad.numpy().reshape(len(z), -1)
        got = b["grads"][k]
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (k, np.abs(got - want).max(), np.abs(want).max())
    want = leaves["means2D"].grad.numpy()[:, :2]
    assert np.abs(b["grads"]["means2D"] - want).max() <= 1e-9 * np.abs(want).max()


@functools.lru_cache(maxsize=None)
def _yardstick(name, form):
    return PR.yardstick(name, form)[0]


@pytest.mark.parametrize("name", PR.case_names())
def test_yardstick_of_a_case(name):
    """The float32 replay's figures of every form of a case stay below the constants the bounds are derived from"""
    for form in PR.yardstick_forms(name):
        for k, v in _yardstick(name, form).items():
            assert v <= PR.YARDSTICK[k] * (1 + 1e-3), (name, form, k, v, PR.YARDSTICK[k])


def test_yardstick_constants():
    """Recomputed over all cases and forms, the float32 replay's largest figures ARE the constants (to their printed digits), and
    the bounds are max(2^-24, 4 x)."""
    worst = {}
    for name in PR.case_names():
        for form in PR.yardstick_forms(name):
            for k, v in _yardstick(name, form).items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(PR.YARDSTICK)
    for k, v in worst.items():
        assert abs(v - PR.YARDSTICK[k]) <= 1e-3 * PR.YARDSTICK[k], (k, v, PR.YARDSTICK[k])
        assert PR.bounds()[k] == max(2.0 ** -24, 4.0 * PR.YARDSTICK[k])


@pytest.mark.parametrize("name", PR.case_names())
def test_undecided_cap(name):
    """From the reference alone: per discrete value, at most 2 % of the visible Gaussians of every case and form are undecided."""
    for form in PR.yardstick_forms(name):
        ref = PR.forward(PR.case_inputs(name, form), np.float64)
        vis = ref["visible"][1]
        n = int(ref["visible"][0].sum())
        for k, u in PR.undecided(ref).items():
            cnt = int((u & (vis | (k in ("front", "visible")))).sum())
            assert cnt <= PR.UNDECIDED_CAP * n, (name, form, k, cnt, n)


def test_edge_scene_sits_where_it_was_put():
    """The hand-built Gaussians are clearly on one side of their threshold or exactly on it (then undecided)."""
    inp = PR.case_inputs("edge", "aa")
    ref = PR.forward(inp, np.float64)
    u = PR.undecided(ref)
    lo, hi = ref["front"]
    assert list(lo[:6]) == [False, False, True, False, False, True] and list(hi[:6]) == [False, True, True, False, False, True]
    assert u["front"].sum() == 1 and not ref["visible"][1][[0, 3, 4]].any()
    inx, iny = ref["in_x"][0], ref["in_y"][0]
    assert list(inx[6:12]) == [False, False, True, True, False, False] and list(iny[6:12]) == [True, True, False, False, False, False]
    assert not u["in_x"][6:12].any() and not u["in_y"][6:12].any() and ref["visible"][0][6:12].all()
    # opacity below / at / above 1 / 255 (the box opens at 255 op > e^-0.01: at 1 / 255 it is open), zero opacity
    base = PR.forward(PR.case_inputs("edge", "base"), np.float64)
    assert list(base["open"][0][12:17]) == [False, True, True, False, True] and not PR.undecided(base)["open"][12:17].any()
    assert ref["radius"][0][17] > max(PR.EDGE_W, PR.EDGE_H) and ref["visible"][0][17]
    assert not ref["visible"][1][18:20].any()                                            # far off screen
    assert not ref["aa_free"][1][20] and not u["aa_free"][20] and ref["visible"][0][20]  # AA at its floor
    assert abs(ref["conic"][20, 0] - 1.0 / 0.3) < 1e-3                                   # the 0.3 dilation is all there is
    cl = ref["clamp"][0]
    assert cl[31, 0] and not cl[31, 1] and cl[32, 1] and cl[32, 2] and cl[34].all()
    gx, gy = (PR.EDGE_W + 15) // 16, (PR.EDGE_H + 15) // 16
    assert PR.EDGE_W % 16 and PR.EDGE_H % 16 and (ref["rect"][1][17] == [0, 0, gx, gy]).all()


@pytest.mark.parametrize("name", ["needles", "needles_08"])
def test_stage_table(name):
    """The per-stage table of profiles/projection_replay.txt comes from PR.stage_table: every stage the backward returns is in it,
    finite, S-relative within the yardstick's order (a few roundings) - and on the needles the per-tensor rel-L2 first leaves the
    1e-6 range at det = a c - b^2, not before."""
    inp = PR.case_inputs(name, "base")
    s32, s64, mag = PR.synthetic_sums(inp, PR.forward(inp, np.float64))
    table, n = PR.stage_table(inp, s32, s64, mag)
    labels = [t[0] for t in table]
    assert n > 5000 and all("bwd " + st in labels for st in PR.STAGES)
    for label, fig, l2 in table:
        assert np.isfinite(fig) and np.isfinite(l2) and fig <= 1e-6, (label, fig, l2)
    d = {t[0]: t[2] for t in table}
    assert max(d["fwd Sigma"], d["fwd cov2D a0"], d["fwd cov2D b"], d["fwd cov2D c0"]) < 1e-6 < d["fwd det"] < d["fwd conic"]
    assert len(PR.format_stage_table(table, n, name)) == len(table) + 1
