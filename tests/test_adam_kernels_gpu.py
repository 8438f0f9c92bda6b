"""k_adam (csrc/adam.hip: the dense and the visibility-masked one-launch Adam, the kernel every folded form of the optimizer
step is held bit-equal to) against the float64 restatement of tests/adam_reference.py, at every size and path of the kernel:
one thread, one 16-byte piece, a piece and a tail, one / two / three workgroups and one element more, tensors on and off the
vector path, misaligned views, empty tensors, 8 / 9 / 11 tensors per step, a step number of 30 000, masks whose 16-byte pieces
straddle a visible and an invisible row.

The bar, per tensor and for p, exp_avg and exp_avg_sq alike: max-abs error <= 4 E32 + 2^-23 max|x64| (adam_reference.tolerance),
E32 being the error of a float32 evaluation with stock torch ops on the same inputs - computed here, never taken from the
kernel.  tests/test_adam_reference_cpu.py shows on these very inputs that the bar passes that float32 evaluation and rejects
eps inside the square root, either bias correction missing, swapped betas, a bias-corrected sparse step and a mask indexed by
element."""
import ctypes as C

import pytest
import torch

import adam_reference as R

pytestmark = pytest.mark.gpu

NAMES = ("p", "exp_avg", "exp_avg_sq")


def _run_fused(inputs, hp, preset=None):
    """FusedAdam over one group per tensor, every gradient step of `inputs`.  -> (params, optimizer).  preset: per tensor
    (step, exp_avg, exp_avg_sq) to start from."""
    from diff_gaussian_rasterization import FusedAdam
    params = [p0.clone().cuda().requires_grad_(True) for p0, _, _, _ in inputs]
    opt = FusedAdam([{"params": [p], "lr": lr} for p, (_, _, _, lr) in zip(params, inputs)], lr=0.0,
                    betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    if preset is not None:
        for p, (step, m, v) in zip(params, preset):
            opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m.clone().cuda(), "exp_avg_sq": v.clone().cuda()}
    grads = [g.cuda() for _, g, _, _ in inputs]
    for t in range(grads[0].shape[0]):
        for p, g in zip(params, grads):
            p.grad = g[t]
        opt.step()
    torch.cuda.synchronize()
    return params, opt


def _state(params, opt):
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in params]


def _hold(label, got, entry, shape):
    """Prints E32 and the kernel's error for p / exp_avg / exp_avg_sq of one tensor, then asserts the bar."""
    errs = [R.max_err(x, r) for x, r in zip(got, entry["ref"])]
    print(f"{label} {tuple(shape)}: " + "  ".join(f"{n} E32 {e32:.3e} kernel {e:.3e} bar {t:.3e}"
                                                   for n, e32, e, t in zip(NAMES, entry["e32"], errs, entry["tol"])))
    for n, e, t in zip(NAMES, errs, entry["tol"]):
        assert e <= t, (label, tuple(shape), n, e, t)


@pytest.mark.parametrize("name", list(R.dense_cases()))
def test_dense_adam_matches_float64(name):
    """Every dense case of adam_reference.dense_cases(): element counts 1 .. 12291 around the piece and workgroup boundaries, model
    -shaped sets for P = 1, 2, 1001, 1364 (every tensor on the 16-byte path), 1366 (all but two off it), 8 / 9 / 11 tensors per
    step (one full launch, two launches), a set whose third tensor is empty, 40 steps, and eps = 1e-8 with betas (0.8, 0.99).
    Besides the bar: every state's step count advanced once per step, elements whose gradient was always 0 keep the parameter's
    bits and m = v = 0, and a second run gives the same bits.

    Measured on an MI355X, max-abs error against float64 as E32 / kernel, worst case of each class (p; exp_avg; exp_avg_sq):
      n-sweep (n,), 6 steps            5.7e-07 / 5.7e-07;  2.0e-06 / 2.0e-06;  5.9e-06 / 4.4e-06
      model sets (P, 3)                1.5e-06 / 1.5e-06;  2.8e-06 / 2.8e-06;  6.3e-05 / 5.4e-05     (6 and 40 steps, both
      model sets (P, 1, 3)             1.2e-06 / 1.2e-06;  2.6e-06 / 2.6e-06;  5.2e-05 / 5.1e-05      hyper-parameter sets;
      model sets (P, 15, 3)            1.8e-06 / 1.8e-06;  4.1e-06 / 4.1e-06;  8.0e-05 / 6.2e-05      the 40-step run is the
      model sets (P, 1)                1.3e-06 / 1.3e-06;  3.0e-06 / 3.0e-06;  6.0e-05 / 5.7e-05      worst of each)
      model sets (P, 4)                1.4e-06 / 1.4e-06;  3.6e-06 / 3.6e-06;  7.1e-05 / 5.8e-05
      8 / 9 / 11 tensors, 3 steps      2.9e-07 / 2.9e-07;  9.9e-07 / 9.9e-07;  2.4e-06 / 3.4e-06
      empty third, 3 steps             3.2e-07 / 3.2e-07;  9.5e-07 / 9.5e-07;  1.3e-06 / 1.8e-06
    The kernel's error never exceeded 0.54 of its bar.  (p: both float32 evaluations round the parameter to the same bits - the
    difference between their updates is far below its spacing - so the two columns agree.)"""
    case = R.dense_cases()[name]
    inputs = R.case_inputs(case)
    ref = R.dense_reference(inputs, hp=case["hp"])
    params, opt = _run_fused(inputs, case["hp"])
    got = _state(params, opt)
    assert len(opt.state) == len(inputs)
    for p in params:
        assert int(opt.state[p]["step"]) == case["steps"]
    for (p0, g, info, lr), entry, x in zip(inputs, ref, got):
        _hold(name, x, entry, p0.shape)
        z = info["always_zero"]
        assert torch.equal(x[0].reshape(-1)[z], p0.reshape(-1)[z])                    # 0 / (0 + eps) is 0: not a bit moves
        assert not x[1].reshape(-1)[z].any() and not x[2].reshape(-1)[z].any()
    again = _state(*_run_fused(inputs, case["hp"]))
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_first_step_moves_every_parameter_by_lr():
    """After step 1 with eps = 1e-15 the bias-corrected update is lr g / (|g| + eps): |dp| = lr wherever |g| >= 1e-6, within
    2^-21 lr (m, g g (1 - beta2), its sqrt, the two bias factors, the quotient and the step size round eight times or so at
    2^-24 each).  Read off directly on parameters that start at 0, where the stored value IS the step.  On N(0, 1) parameters a
    float32 of size 1 cannot hold a change of 1e-4 to that precision (its own rounding is 2^-24 |p|), so there the statement is
    the sharpest one the storage allows: the new parameter is the float32 rounding of p - s for some s within 2^-21 lr of
    +-lr.  Measured on an MI355X: | |dp| - lr | <= 0.59 x 2^-21 lr on every tensor."""
    inputs = R.case_inputs(R.dense_cases()["model1366"]) + R.case_inputs(R.dense_cases()["n4097"])
    for zero_start in (True, False):
        ins = [((torch.zeros_like(p0) if zero_start else p0), g[:1], info, lr) for p0, g, info, lr in inputs]
        params, opt = _run_fused(ins, R.DEFAULT)
        for (p0, g, _, lr), p in zip(ins, params):
            big = g[0].abs() >= 1e-6
            assert int(big.sum()) > 0.6 * big.numel() - 2
            new, old, s = p.detach().cpu()[big], p0[big].double(), torch.sign(g[0][big]).double()
            if zero_start:
                dev = float(((new.double().abs() - lr).abs()).max())
                print(f"{tuple(p0.shape)} lr {lr}: | |dp| - lr | max {dev / lr * 2 ** 21:.3f} x 2^-21 lr")
                assert dev <= 2.0 ** -21 * lr
                assert torch.equal(torch.sign(new).double(), -s)
            a, b = (old - s * lr * (1 + 2.0 ** -21)).float(), (old - s * lr * (1 - 2.0 ** -21)).float()
            assert bool(((new >= torch.minimum(a, b)) & (new <= torch.maximum(a, b))).all())


def _raw_dense(ts, lrs, steps, hp=R.DEFAULT):
    """gsr_adam_step through the C ABI on [(p, g, m, v)] device tensors (views allowed) -> return code."""
    from diff_gaussian_rasterization import _C
    n = len(ts)
    arr = [(C.c_void_p * n)(*[t[k].data_ptr() for t in ts]) for k in range(4)]
    num = (C.c_int64 * n)(*[t[0].numel() for t in ts])
    with _C.on_device(torch.device("cuda", torch.cuda.current_device())):
        return _C.check(_C.lib().gsr_adam_step(n, arr[0], arr[1], arr[2], arr[3], num, (C.c_float * n)(*lrs),
                                               (C.c_int64 * n)(*steps), hp["beta1"], hp["beta2"], hp["eps"], _C._stream()))


@pytest.mark.parametrize("which", ["p", "exp_avg_sq", "all"])
def test_misaligned_views_take_the_scalar_path_with_the_same_bits(which):
    """n % 4 == 0, but the parameter (or only exp_avg_sq, or all four tensors) starts 4 bytes into its storage: the kernel must
    see that no 16-byte access is possible and give exactly what the aligned run of the same values gives."""
    n = 4100                                     # two workgroups, the second one nearly empty
    p0, g, _, lr = R.case_inputs(dict(shapes=[(n,)], lrs=[0.005], steps=3, seed=41))[0]
    out = {}
    for shifted in (False, True):
        def place(x, name):
            off = 1 if shifted and which in (name, "all") else 0
            buf = torch.full((n + 8,), float("nan"), device="cuda")
            buf[off:off + n] = x.cuda()
            return buf, buf[off:off + n]
        (pb, p), (mb, m), (vb, v) = place(p0, "p"), place(torch.zeros(n), "exp_avg"), place(torch.zeros(n), "exp_avg_sq")
        if shifted:
            assert (p.data_ptr() % 16 == 4) == (which in ("p", "all")) and (v.data_ptr() % 16 == 4) == (which != "p")
        for t in range(3):
            gb, gt = place(g[t], "g")
            assert _raw_dense([(p, gt, m, v)], [lr], [t + 1]) == 0
        torch.cuda.synchronize()
        out[shifted] = (p.cpu(), m.cpu(), v.cpu())
        for buf, view in ((pb, p), (mb, m), (vb, v)):       # nothing outside the view was written
            outside = torch.ones(n + 8, dtype=torch.bool)
            outside[view.storage_offset():view.storage_offset() + n] = False
            assert bool(torch.isnan(buf.cpu()[outside]).all())
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    ref = R.dense_reference([(p0, g, None, lr)])[0]
    _hold("misaligned " + which, out[True], ref, p0.shape)


def test_empty_tensor_in_a_launch_and_an_empty_launch():
    """A launch of six whose third tensor has no elements (a model pruned to nothing in one group): returns 0, the five others
    are updated as if it were not there.  A launch of nothing but empty tensors, and one of no tensors, return 0 too."""
    case = R.dense_cases()["empty_third"]
    inputs = R.case_inputs(case)
    ref = R.dense_reference(inputs, hp=case["hp"])
    ts = [(p0.clone().cuda(), None, torch.zeros_like(p0).cuda(), torch.zeros_like(p0).cuda()) for p0, _, _, _ in inputs]
    assert ts[2][0].numel() == 0
    for t in range(case["steps"]):
        step = [(p, g[t].cuda(), m, v) for (p, _, m, v), (_, g, _, _) in zip(ts, inputs)]
        assert _raw_dense(step, case["lrs"], [t + 1] * 6) == 0
    torch.cuda.synchronize()
    for (p0, _, _, _), entry, (p, _, m, v) in zip(inputs, ref, ts):
        _hold("empty third (C ABI)", (p.cpu(), m.cpu(), v.cpu()), entry, p0.shape)
    e = torch.zeros(0, device="cuda")
    assert _raw_dense([(e, e, e, e)] * 3, [0.1] * 3, [1] * 3) == 0
    assert _raw_dense([], [], []) == 0


@pytest.mark.parametrize("n", [1028, 1030])
def test_step_jump_to_30000(n):
    """Parameters and moments of the float64 reference at step 29 999 (cast to float32), state["step"] = 29999, three more
    steps: the host forms 1 - 0.9^30000 and 1 - 0.999^30000 and the kernel starts from moments that were never zero.  Measured on an MI355X (E32 / kernel): p 2.2e-06 / 2.2e-06, exp_avg
    1.5e-06 / 1.5e-06, exp_avg_sq 4.1e-04 / 3.3e-04 (of values up to 2.9e3)."""
    p, m, v, grads, info = R.step_jump_state(n)
    p32, m32, v32 = p.float(), m.float(), v.float()
    inputs = [(p32, grads, info, R.JUMP_LR)]
    ref = R.dense_reference(inputs, first_step=R.JUMP_STEP + 1, m0=[m32], v0=[v32])
    params, opt = _run_fused(inputs, R.DEFAULT, preset=[(R.JUMP_STEP, m32, v32)])
    assert int(opt.state[params[0]]["step"]) == R.JUMP_STEP + 3
    _hold("step jump", _state(params, opt)[0], ref[0], p32.shape)
    z = info["always_zero"]
    assert torch.equal(params[0].detach().cpu()[z], p32[z])


def _run_sparse(inputs, vis_dev, N, snapshots=(1, 6)):
    from diff_gaussian_rasterization import SparseGaussianAdam
    params = [p0.clone().cuda().requires_grad_(True) for p0, _, _, _, _ in inputs]
    opt = SparseGaussianAdam([{"params": [p], "lr": lr} for p, (_, _, _, lr, _) in zip(params, inputs)], lr=0.0, eps=1e-15)
    grads = [g.cuda() for _, g, _, _, _ in inputs]
    out = {}
    for t in range(max(snapshots)):
        for p, g in zip(params, grads):
            p.grad = g[t]
        opt.step(vis_dev, N)
        if t + 1 in snapshots:
            torch.cuda.synchronize()
            out[t + 1] = _state(params, opt)
    return out


@pytest.mark.parametrize("N", R.SPARSE_N)
def test_sparse_adam_matches_float64(N):
    """SparseGaussianAdam on the six model tensors of N Gaussians, every visibility pattern (all, none, alternating rows - at N =
    1364 every 16-byte piece of the 3- and 45-wide tensors then straddles a visible and an invisible row -, only the last row,
    only the first, random 60 %), after 1 and after 6 steps: visible rows within the bar of sparse_step in float64, invisible
    rows bit-identical in p, exp_avg and exp_avg_sq (with no row visible: nothing moves at all), the mask as torch.bool and as
    torch.uint8 with equal results.

    Measured on an MI355X, max-abs error against float64 as E32 / kernel, worst over every N, pattern and both step counts (p;
    exp_avg; exp_avg_sq):
      (N, 3)       5.3e-07 / 5.3e-07;  3.1e-06 / 3.2e-06;  7.5e-06 / 5.3e-06
      (N, 1, 3)    4.5e-07 / 4.5e-07;  3.8e-06 / 2.6e-06;  4.7e-06 / 5.2e-06
      (N, 15, 3)   6.6e-07 / 6.6e-07;  5.0e-06 / 3.5e-06;  7.7e-06 / 6.5e-06
      (N, 1)       4.2e-07 / 4.2e-07;  2.5e-06 / 2.5e-06;  4.1e-06 / 3.7e-06
      (N, 4)       5.0e-07 / 5.0e-07;  3.5e-06 / 3.8e-06;  5.9e-06 / 4.6e-06
    The kernel's error never exceeded 0.62 of its bar."""
    inputs = R.sparse_inputs(N)
    for pattern in R.VISIBILITY:
        vis = R.visibility(N, pattern, N)
        got = _run_sparse(inputs, vis.cuda(), N)
        as_u8 = _run_sparse(inputs, vis.to(torch.uint8).cuda(), N)
        for steps in (1, 6):
            ref = R.sparse_reference(inputs, vis, steps)
            for (p0, g, info, lr, row), entry, x, y in zip(inputs, ref, got[steps], as_u8[steps]):
                _hold(f"sparse N={N} {pattern} {steps} step(s)", x, entry, p0.shape)
                inv = ~vis
                assert torch.equal(x[0][inv], p0[inv]) and not x[1][inv].any() and not x[2][inv].any()
                for a, b in zip(x, y):
                    assert torch.equal(a, b)
                if pattern == "none":
                    assert torch.equal(x[0], p0)
                if vis.any():
                    assert not torch.equal(x[0][vis], p0[vis])
