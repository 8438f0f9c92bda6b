"""tests/adam_reference.py without a GPU: the float64 steps against torch.optim.Adam and against the masked restatement of
tests/test_loss_adam_gpu.py, and the mutation check of the bar the kernel tests use (4 E32 + 2^-23 max|x64|, adam_reference.
tolerance): on every input case of tests/test_adam_kernels_gpu.py the float32 reference passes it and every deliberately wrong
step misses it on at least one tensor.  Also the optimizers' refusal of hyper-parameters one launch cannot carry."""
import pytest
import torch

import adam_reference as R


def test_dense_step_is_torch_adam_in_float64():
    """50 steps on the model-shaped inputs, both hyper-parameter sets: parameters and both moments equal torch.optim.Adam on
    float64 tensors to 1e-13 relative, per tensor and element by element."""
    for hp in (R.DEFAULT, R.OTHER):
        inputs = [R.make_inputs(s, 50, 900 + j) + (lr,) for j, (s, lr) in enumerate(zip(R.model_shapes(211), R.LRS))]
        params = [p0.double().clone().requires_grad_(True) for p0, _, _, _ in inputs]
        opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, (_, _, _, lr) in zip(params, inputs)], lr=0.0,
                               betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
        for t in range(50):
            for p, (_, g, _, _) in zip(params, inputs):
                p.grad = g[t].double()
            opt.step()
        for p, (p0, g, _, lr) in zip(params, inputs):
            ref = R.run_dense(R.dense_step, p0, g, lr, hp=hp)
            st = opt.state[p]
            for what, mine, theirs in zip("pmv", ref, (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
                assert mine.dtype == torch.float64
                diff = (mine - theirs).abs()
                assert float(diff.max()) <= 1e-13 * float(theirs.abs().max()), what
                # ... and element by element; the first moment is a signed sum whose terms cancel on purpose here, so its own
                # size is no measure of its rounding: it is held relative to the largest gradient the element has seen
                scale = g.double().abs().amax(dim=0) if what == "m" else theirs.abs()
                assert bool((diff <= 1e-13 * scale).all()), what


def test_sparse_step_is_the_masked_restatement():
    """sparse_step against the expression test_sparse_adam_touches_only_visible_rows restates (0.9 m + 0.1 g, 0.999 v + 0.001 g g,
    p - lr m / (sqrt(v) + 1e-15), torch.where over the row mask), evaluated in float64."""
    N = 777
    vis = R.visibility(N, "random", N)
    for p0, grads, _, lr, row in R.sparse_inputs(N, steps=3):
        m, v, cur = torch.zeros_like(p0).double(), torch.zeros_like(p0).double(), p0.double()
        for g in grads.double():
            mask = vis.view(N, *([1] * (g.dim() - 1))).expand_as(g)
            m_new = 0.9 * m + 0.1 * g
            v_new = 0.999 * v + 0.001 * g * g
            upd = cur - lr * m_new / (v_new.sqrt() + 1e-15)
            m, v, cur = torch.where(mask, m_new, m), torch.where(mask, v_new, v), torch.where(mask, upd, cur)
        ref = R.run_sparse(R.sparse_step, p0, grads, lr, vis, row)
        for what, mine, theirs in zip("pmv", ref, (cur, m, v)):
            diff = (mine - theirs).abs()
            assert float(diff.max()) <= 1e-13 * float(theirs.abs().max()), what
            # element by element, each against the size of its own terms (see the dense test): a parameter near zero is |p0| plus
            # steps of lr, a first moment a signed sum of gradients
            scale = {"p": theirs.abs() + 3 * lr, "m": grads.double().abs().amax(dim=0), "v": theirs.abs()}[what]
            assert bool((diff <= 1e-13 * scale).all()), what
        inv = ~vis
        assert torch.equal(ref[0][inv], p0.double()[inv]) and not ref[1][inv].any() and not ref[2][inv].any()


def test_inputs_have_what_the_kernel_tests_rely_on():
    p0, g, info = R.make_inputs((1366, 15, 3), 40, 5)
    flat = g.reshape(40, -1)
    assert not flat[:, info["always_zero"]].any() and flat[:, info["always_zero"]].shape[1] == 1366 * 45 // 8
    later = flat[:, info["zero_later"]]
    assert later[:info["zero_from"]].abs().min() > 0 and not later[info["zero_from"]:].any()
    mag = flat[flat != 0].abs()
    assert 1e-8 <= float(mag.min()) < 1e-7 and 1e1 < float(mag.max()) <= 1e2
    assert info["always_zero"].start % 45 != 0                     # the block starts inside a row
    # signs that make the first moment cancel: elements alternating every step, elements flipping once late in the run
    s = torch.sign(flat[:, :info["always_zero"].start])
    assert bool(((s[1:] == -s[:-1]).all(dim=0)).any())
    assert bool((((s[:27] == s[0]).all(dim=0)) & ((s[27:] == -s[0]).all(dim=0))).any())
    for n in (1, 3):
        assert R.zero_blocks(n) == (slice(n // 2, n // 2), slice(n // 2, n // 2))
    assert torch.equal(R.make_inputs((5,), 6, 108)[1], R.make_inputs((5,), 6, 108)[1])      # seeded


@pytest.mark.parametrize("name", list(R.dense_cases()))
def test_bar_accepts_fp32_and_rejects_every_wrong_dense_step(name):
    case = R.dense_cases()[name]
    inputs = R.case_inputs(case)
    ref = R.dense_reference(inputs, hp=case["hp"])
    for (p0, g, _, lr), entry in zip(inputs, ref):
        assert not R.exceeds(R.run_dense(R.dense_step_fp32, p0, g, lr, hp=case["hp"]), entry)
    for variant, fn in R.DENSE_WRONG.items():
        assert any(R.exceeds(R.run_dense(fn, p0, g, lr, hp=case["hp"]), entry)
                   for (p0, g, _, lr), entry in zip(inputs, ref)), variant


@pytest.mark.parametrize("n", [1028, 1030])
def test_bar_at_the_step_jump(n):
    """Steps 30 000 .. 30 002 from the float64 state of step 29 999.  The two variants that drop a bias correction are not
    wrong there - 1 - 0.9^30000 is 1 and 1 - 0.999^30000 is 1 - 9e-14, both 1.0f - so they are the one pair of (case, variant)
    this check leaves out; what the case adds to the kernel test is the host's pow() at a large step and moments that are not
    zero-initialised."""
    p, m, v, grads, _ = R.step_jump_state(n)
    assert float(1.0 - 0.999 ** 30000) == pytest.approx(1.0, abs=1e-12)
    p32, m32, v32 = p.float(), m.float(), v.float()
    kw = dict(first_step=R.JUMP_STEP + 1, m0=m32, v0=v32)
    ref = R.run_dense(R.dense_step, p32, grads, R.JUMP_LR, **kw)
    got = R.run_dense(R.dense_step_fp32, p32, grads, R.JUMP_LR, **kw)
    entry = dict(ref=ref, tol=[R.tolerance(R.max_err(a, b), b) for a, b in zip(got, ref)])
    assert not R.exceeds(got, entry)
    for variant in ("eps_inside_sqrt", "betas_swapped"):
        assert R.exceeds(R.run_dense(R.DENSE_WRONG[variant], p32, grads, R.JUMP_LR, **kw), entry), variant


@pytest.mark.parametrize("N", R.SPARSE_N)
def test_bar_accepts_fp32_and_rejects_every_wrong_sparse_step(N):
    """Every visibility pattern, after 1 and after 6 steps.  Left out, because the variant IS the right step there: everything
    when no row is visible (nothing moves), `visible` indexed by element when all rows are visible or N = 1."""
    inputs = R.sparse_inputs(N)
    for pattern in R.VISIBILITY:
        vis = R.visibility(N, pattern, N)
        for steps in (1, 6):
            ref = R.sparse_reference(inputs, vis, steps)
            for (p0, g, _, lr, row), entry in zip(inputs, ref):
                assert not R.exceeds(R.run_sparse(R.sparse_step_fp32, p0, g[:steps], lr, vis, row), entry)
            if not vis.any():
                continue
            for variant, fn in R.SPARSE_WRONG.items():
                if variant == "visible_by_element" and bool(vis.all()):
                    continue
                assert any(R.exceeds(R.run_sparse(fn, p0, g[:steps], lr, vis, row, with_step=True), entry)
                           for (p0, g, _, lr, row), entry in zip(inputs, ref)), (pattern, steps, variant)


# ---- the optimizers refuse hyper-parameters that one launch cannot carry (host-side: before any device call) ----
def _groups(**over):
    ps = [torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(5, 1))]
    for p in ps:
        p.grad = torch.ones_like(p)
    groups = [{"params": [ps[0]], "lr": 0.01, "name": "xyz"}, {"params": [ps[1]], "lr": 0.02, "name": "opacity"}]
    groups[1].update(over)
    return groups


@pytest.mark.parametrize("over", [dict(betas=(0.8, 0.999)), dict(betas=(0.9, 0.99)), dict(eps=1e-8)])
def test_optimizers_refuse_groups_whose_betas_or_eps_differ(over):
    from diff_gaussian_rasterization import _C, FusedAdam, SparseGaussianAdam
    dense = FusedAdam(_groups(**over), lr=0.0, eps=1e-15)
    with pytest.raises(_C.GsrError, match="group 1 .*opacity"):
        dense.step()
    sparse = SparseGaussianAdam(_groups(**over), lr=0.0, eps=1e-15)
    with pytest.raises(_C.GsrError, match="group 1 .*opacity"):
        sparse.step(torch.ones(5, dtype=torch.bool), 5)
    with pytest.raises(_C.GsrError, match="group 1 .*opacity"):        # restricted to the other group: still one optimizer
        dense.step(only=("xyz",))


def test_sparse_optimizer_refuses_other_betas_and_uniform_groups_reach_the_device_check():
    from diff_gaussian_rasterization import _C, FusedAdam, SparseGaussianAdam
    sparse = SparseGaussianAdam(_groups(), lr=0.0, eps=1e-15)
    for g in sparse.param_groups:
        g["betas"] = (0.8, 0.99)
    with pytest.raises(_C.GsrError, match=r"betas=\(0\.9, 0\.999\) only"):
        sparse.step(torch.ones(5, dtype=torch.bool), 5)
    # uniform hyper-parameters pass the check; the next thing in the way of CPU tensors is the "no CPU path" refusal
    for opt, args in ((FusedAdam(_groups(), lr=0.0, betas=(0.8, 0.99), eps=1e-8), ()),
                      (SparseGaussianAdam(_groups(), lr=0.0, eps=1e-15), (torch.ones(5, dtype=torch.bool), 5))):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            opt.step(*args)
