"""Plain restatement of the two Adam updates of csrc/adam.hip for the optimizer tests, and the inputs those tests share.
Nothing here calls the HIP path.

  dense_step / sparse_step      float64, the reference the kernels are held to
  dense_step_fp32 / sparse_step_fp32
                                the same two steps in float32 with stock torch ops (torch.optim.Adam's own operation order:
                                lerp, addcmul, a division by sqrt(bias_correction2)) - what float32 reaches on an input, NOT the
                                kernel's operation order (explicit fma, reciprocal bias factor)
  DENSE_WRONG / SPARSE_WRONG    float32 steps that are deliberately not Adam; only there to show that `tolerance` rejects them
  make_inputs, visibility       the seeded inputs (tests/test_adam_reference_cpu.py and tests/test_adam_kernels_gpu.py)

All steps are functional: they return new (p, m, v) and leave their arguments alone."""
import functools
import math

import torch

LRS = (0.00016, 0.0025, 0.000125, 0.025, 0.005, 0.001)          # xyz, f_dc, f_rest, opacity, scaling, rotation
DEFAULT = dict(beta1=0.9, beta2=0.999, eps=1e-15)                 # the model's optimizer (Adam(l, lr=0.0, eps=1e-15))
OTHER = dict(beta1=0.8, beta2=0.99, eps=1e-8)


def model_shapes(P):
    return [(P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4)]


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def dense_step(p, m, v, g, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    """One step of torch.optim.Adam (no amsgrad, no weight decay) in float64; `step` is the 1-based number of THIS step."""
    p, m, v, g = (t.detach().double() for t in (p, m, v, g))
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def _row_mask(visible, like, row):
    n = like.numel()
    assert n % row == 0 and visible.numel() == n // row
    return (visible.reshape(-1) != 0).repeat_interleave(row).reshape(like.shape)


def sparse_step(p, m, v, g, lr, visible, row, beta1=0.9, beta2=0.999, eps=1e-15):
    """The visibility-masked step as csrc/adam.hip documents it: no bias correction, p -= lr m / (sqrt(v) + eps); the `row`
    consecutive elements of a Gaussian whose visible[] is 0 keep p, m and v."""
    p, m, v, g = (t.detach().double() for t in (p, m, v, g))
    mask = _row_mask(visible, p, row)
    m_new = beta1 * m + (1.0 - beta1) * g
    v_new = beta2 * v + (1.0 - beta2) * g * g
    p_new = p - lr * m_new / (v_new.sqrt() + eps)
    return torch.where(mask, p_new, p), torch.where(mask, m_new, m), torch.where(mask, v_new, v)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 with stock torch ops, and the wrong variants (one body, so that a variant differs from the right step in ONE place)
# ---------------------------------------------------------------------------------------------------------------------------
def _dense32(p, m, v, g, lr, step, beta1=0.9, beta2=0.999, eps=1e-15, eps_in_sqrt=False, no_bc2=False, no_bc1=False,
             swap_betas=False):
    p, m, v, g = (t.detach().float() for t in (p, m, v, g))
    if swap_betas:
        beta1, beta2 = beta2, beta1
    m = torch.lerp(m, g, 1.0 - beta1)
    v = torch.addcmul(v * beta2, g, g, value=1.0 - beta2)
    bc1 = 1.0 if no_bc1 else 1.0 - beta1 ** step
    bc2 = 1.0 if no_bc2 else 1.0 - beta2 ** step
    if eps_in_sqrt:
        denom = (v + eps).sqrt() / math.sqrt(bc2)
    else:
        denom = v.sqrt() / math.sqrt(bc2) + eps
    p = torch.addcdiv(p, m, denom, value=-(lr / bc1))
    return p, m, v


def _sparse32(p, m, v, g, lr, visible, row, beta1=0.9, beta2=0.999, eps=1e-15, step=None, eps_in_sqrt=False,
              swap_betas=False, bias_correction=False, by_element=False):
    p, m, v, g = (t.detach().float() for t in (p, m, v, g))
    if swap_betas:
        beta1, beta2 = beta2, beta1
    if by_element:      # element i looks at visible[i] instead of visible[i / row] (wrapped, where a kernel would run off the end)
        vis = visible.reshape(-1) != 0
        mask = vis[torch.arange(p.numel()) % vis.numel()].reshape(p.shape)
    else:
        mask = _row_mask(visible, p, row)
    m_new = m * beta1 + g * (1.0 - beta1)
    v_new = torch.addcmul(v * beta2, g, g, value=1.0 - beta2)
    bc1 = bc2 = 1.0
    if bias_correction:
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = (v_new + eps).sqrt() if eps_in_sqrt else v_new.sqrt() / math.sqrt(bc2) + eps
    p_new = torch.addcdiv(p, m_new, denom, value=-(lr / bc1))
    return torch.where(mask, p_new, p), torch.where(mask, m_new, m), torch.where(mask, v_new, v)


def dense_step_fp32(p, m, v, g, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    return _dense32(p, m, v, g, lr, step, beta1, beta2, eps)


def sparse_step_fp32(p, m, v, g, lr, visible, row, beta1=0.9, beta2=0.999, eps=1e-15, step=None):
    return _sparse32(p, m, v, g, lr, visible, row, beta1, beta2, eps)


DENSE_WRONG = {
    "eps_inside_sqrt": functools.partial(_dense32, eps_in_sqrt=True),
    "no_bias_correction2": functools.partial(_dense32, no_bc2=True),
    "no_bias_correction1": functools.partial(_dense32, no_bc1=True),
    "betas_swapped": functools.partial(_dense32, swap_betas=True),
}
SPARSE_WRONG = {          # (all take the step number as keyword `step`; only the bias-corrected one uses it)
    "eps_inside_sqrt": functools.partial(_sparse32, eps_in_sqrt=True),
    "betas_swapped": functools.partial(_sparse32, swap_betas=True),
    "bias_corrected": functools.partial(_sparse32, bias_correction=True),
    "visible_by_element": functools.partial(_sparse32, by_element=True),
}


# ---------------------------------------------------------------------------------------------------------------------------
# running a step function over a gradient sequence, and the bar
# ---------------------------------------------------------------------------------------------------------------------------
def run_dense(step_fn, p0, grads, lr, hp=DEFAULT, first_step=1, m0=None, v0=None):
    """-> (p, m, v) after len(grads) steps numbered first_step, first_step + 1, ..."""
    p = p0
    m = torch.zeros_like(p0) if m0 is None else m0
    v = torch.zeros_like(p0) if v0 is None else v0
    for t, g in enumerate(grads):
        p, m, v = step_fn(p, m, v, g, lr, first_step + t, **hp)
    return p, m, v


def run_sparse(step_fn, p0, grads, lr, visible, row, hp=DEFAULT, with_step=False):
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(grads):
        kw = dict(step=t + 1) if with_step else {}
        p, m, v = step_fn(p, m, v, g, lr, visible, row, **hp, **kw)
    return p, m, v


def max_err(x, x64):
    return float((x.detach().double().cpu() - x64).abs().max()) if x64.numel() else 0.0


def tolerance(e32, x64):
    """The bar of the kernel tests for one tensor: 4 E32 + 2^-23 max|x64|.  E32 = max_err(fp32 reference, float64 reference) on
    that tensor.  4: another, equally valid float32 operation order; the floor: one final rounding flip when E32 is 0."""
    return 4.0 * e32 + 2.0 ** -23 * (float(x64.abs().max()) if x64.numel() else 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def zero_blocks(n):
    """(always-zero slice, zero-from-mid-run slice) of the flat element range: an eighth of the tensor each, from one element
    before the middle on (so that they start inside a row and inside a 16-byte piece for the model's row widths); one element
    each for 4 <= n < 8."""
    z = n // 8 if n >= 8 else (1 if n >= 4 else 0)
    a = n // 2 - (1 if n >= 8 else 0)
    return slice(a, a + z), slice(a + z, a + 2 * z)


def make_inputs(shape, steps, seed):
    """-> (p0 [*shape] float32, grads [steps, *shape] float32, info).  Parameters N(0, 1).  Gradient magnitudes 10^(d + u), d a
    decade from -8 .. 1 and u uniform in [0, 1): 1e-8 .. 1e2.  Half of the elements keep their decade for the whole run (so
    some elements only ever see tiny gradients, others only large ones), the other half draws a new one every step.  Signs: a
    quarter of the elements alternates every step, a quarter keeps one sign for two thirds of the run and then flips (the first
    moment cancels and changes sign), the rest is random.  One block has gradient 0 on every step, the next one from the middle
    of the run on (moments decay, the parameter drifts on its momentum).  info: the two blocks as flat slices, `zero_from`."""
    n = 1
    for s in shape:
        n *= int(s)
    gen = torch.Generator().manual_seed(int(seed))
    p0 = torch.randn(n, generator=gen)
    base = torch.randint(-8, 2, (n,), generator=gen)
    redraw = torch.rand(n, generator=gen) < 0.5
    dec = torch.where(redraw[None, :], torch.randint(-8, 2, (steps, n), generator=gen), base[None, :].expand(steps, n))
    mag = 10.0 ** (dec.double() + torch.rand(steps, n, generator=gen, dtype=torch.float64))
    kind = torch.randint(0, 4, (n,), generator=gen)
    sign = torch.where(torch.rand(steps, n, generator=gen) < 0.5, -1.0, 1.0).double()
    first = sign[0:1].expand(steps, n)
    t = torch.arange(steps)[:, None]
    flip_at = (2 * steps + 2) // 3
    sign = torch.where(kind[None, :] == 1, first * torch.where(t % 2 == 0, 1.0, -1.0).double(), sign)
    sign = torch.where(kind[None, :] == 2, first * torch.where(t < flip_at, 1.0, -1.0).double(), sign)
    g = (sign * mag).float()
    always, later = zero_blocks(n)
    zero_from = max(1, steps // 2)
    g[:, always] = 0.0
    g[zero_from:, later] = 0.0
    info = dict(always_zero=always, zero_later=later, zero_from=zero_from)
    return p0.reshape(shape), g.reshape(steps, *shape), info


VISIBILITY = ("all", "none", "alternating", "last", "first", "random")


def visibility(N, pattern, seed=0):
    """bool [N]"""
    vis = torch.zeros(N, dtype=torch.bool)
    if pattern == "all":
        vis[:] = True
    elif pattern == "alternating":
        vis[::2] = True
    elif pattern == "last":
        vis[N - 1] = True
    elif pattern == "first":
        vis[0] = True
    elif pattern == "random":
        vis = torch.rand(N, generator=torch.Generator().manual_seed(1000 + int(seed))) < 0.6
    elif pattern != "none":
        raise ValueError(pattern)
    return vis


# the step jump: moments and parameters of a long run, taken from the float64 reference
JUMP_STEP, JUMP_LR, JUMP_CYCLE = 29999, 0.001, 64


@functools.lru_cache(maxsize=None)
def step_jump_state(n, seed=77):
    """(p, m, v) of the float64 reference after JUMP_STEP steps on n elements (the gradient sequence of make_inputs((n,),
    JUMP_CYCLE, seed), repeated), and the gradients of the three steps that follow."""
    p0, g, info = make_inputs((n,), JUMP_CYCLE, seed)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, JUMP_STEP + 1):
        p, m, v = dense_step(p, m, v, g[(t - 1) % JUMP_CYCLE], JUMP_LR, t, **DEFAULT)
    nxt = torch.stack([g[(JUMP_STEP + k) % JUMP_CYCLE] for k in range(3)])
    return p, m, v, nxt, info


# ---------------------------------------------------------------------------------------------------------------------------
# the dense input cases (shared by the CPU mutation check and the GPU test): name -> dict(shapes, lrs, steps, hp, seed)
# ---------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 1023, 1024, 4095, 4096, 4097, 8192, 8193, 12291)
MODEL_P = (1, 2, 1001, 1364, 1366)
SHORT_RUN = 6
# Seeds.  A wrong variant can only be told from Adam on an element whose gradients make it differ: eps inside the square root
# with eps = 1e-15 needs an element that only ever saw |g| << 1e-5.  A tensor of one to five elements has such an element for
# some seeds and not for others; these are seeds at which tests/test_adam_reference_cpu.py finds every variant rejected (the
# inputs are chosen, the bar is not touched).  Every other case uses its default seed.
SIZE_SEED = {1: 103, 3: 104, 4: 104, 5: 108}
MODEL_SEED = {}


def dense_cases():
    cases = {}
    for i, n in enumerate(SIZES):
        cases[f"n{n}"] = dict(shapes=[(n,)], lrs=[LRS[i % 6]], steps=SHORT_RUN, hp=DEFAULT, seed=SIZE_SEED.get(n, 100 + n))
    for P in MODEL_P:
        cases[f"model{P}"] = dict(shapes=model_shapes(P), lrs=list(LRS), steps=SHORT_RUN, hp=DEFAULT,
                                  seed=MODEL_SEED.get(P, 200 + P))
    for k in (8, 9, 11):        # one full launch; two launches (8 + 1, 8 + 3)
        cases[f"tensors{k}"] = dict(shapes=[(37 + 5 * j, 1 + j % 4) for j in range(k)], lrs=[LRS[j % 6] for j in range(k)],
                                    steps=3, hp=DEFAULT, seed=300 + k)
    shapes = model_shapes(52)
    shapes[2] = (0, 15, 3)
    cases["empty_third"] = dict(shapes=shapes, lrs=list(LRS), steps=3, hp=DEFAULT, seed=400)
    cases["model1366_40steps"] = dict(shapes=model_shapes(1366), lrs=list(LRS), steps=40, hp=DEFAULT, seed=500)
    cases["model1366_other_hp"] = dict(shapes=model_shapes(1366), lrs=list(LRS), steps=SHORT_RUN, hp=OTHER, seed=600)
    return cases


def case_inputs(case):
    """-> [(p0, grads, info, lr)] of a dense case, one entry per tensor (tensor j is seeded case seed + 7919 j)."""
    return [make_inputs(s, case["steps"], case["seed"] + 7919 * j) + (lr,)
            for j, (s, lr) in enumerate(zip(case["shapes"], case["lrs"]))]


SPARSE_N = (1, 4, 777, 1364, 1366)
SPARSE_SEED = {}


def sparse_inputs(N, steps=6):
    """-> [(p0, grads, info, lr, row)] for the six model tensors of N Gaussians."""
    out = []
    for j, (s, lr) in enumerate(zip(model_shapes(N), LRS)):
        p0, g, info = make_inputs(s, steps, SPARSE_SEED.get(N, 700 + N) + 7919 * j)
        out.append((p0, g, info, lr, p0.numel() // N))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# reference results and bars, computed once per case
# ---------------------------------------------------------------------------------------------------------------------------
def _bars(ref64, got32):
    e32 = [max_err(a, b) for a, b in zip(got32, ref64)]
    return e32, [tolerance(e, b) for e, b in zip(e32, ref64)]


def dense_reference(inputs, steps_fn=dense_step, hp=DEFAULT, first_step=1, m0=None, v0=None):
    """inputs: [(p0, grads, info, lr)] -> per tensor dict(ref=(p, m, v) float64, e32=[3], tol=[3])."""
    out = []
    for j, (p0, g, info, lr) in enumerate(inputs):
        kw = dict(hp=hp, first_step=first_step, m0=None if m0 is None else m0[j], v0=None if v0 is None else v0[j])
        ref = run_dense(dense_step, p0, g, lr, **kw)
        e32, tol = _bars(ref, run_dense(dense_step_fp32, p0, g, lr, **kw))
        out.append(dict(ref=ref, e32=e32, tol=tol))
    return out


def sparse_reference(inputs, vis, steps, hp=DEFAULT):
    """inputs: sparse_inputs(N) -> per tensor dict(ref, e32, tol) after the first `steps` steps."""
    out = []
    for p0, g, info, lr, row in inputs:
        ref = run_sparse(sparse_step, p0, g[:steps], lr, vis, row, hp)
        e32, tol = _bars(ref, run_sparse(sparse_step_fp32, p0, g[:steps], lr, vis, row, hp))
        out.append(dict(ref=ref, e32=e32, tol=tol))
    return out


def exceeds(got, entry):
    """Whether (p, m, v) `got` misses the bar of a reference entry on p, m or v."""
    return any(max_err(x, r) > t for x, r, t in zip(got, entry["ref"], entry["tol"]))
