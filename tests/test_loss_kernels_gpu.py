"""The loss kernels of csrc/ssim.hip against the float64 reference of tests/loss_reference.py, pixel by pixel and tile by tile:
k_ssim_fwd (map, the three saved maps, per-tile sums; one and two tiles per workgroup), k_ssim_bwd (map form and fused form),
k_loss_finalize, and the three l1_mean kernels.  Every pixel is held to the first-order bound derived in loss_reference's
docstring (K = 24 roundings per window moment; tests/test_loss_reference_cpu.py shows what float32 uses of it and that a dropped
tap, a shifted halo column and an unmasked row exceed it by orders of magnitude) - no fixed tolerance: on a flat image the float32
error of the map is 100x what it is on noise.

The kernels are called through the C ABI on buffers this file owns: every output is NaN before the call and sits between two
guards of 64 sentinel floats, so a pixel or tile that was never written, and a write outside the buffer, show whatever the
allocator happened to hold.  (k_ssim_fwd takes `ssim_map` and `partials`, but no entry point of the C ABI passes both: what can
be reached is held bit for bit - the map with and without the saved maps, the saved maps with and without the per-tile sums.)
Run with -s for the largest error / bound of every case.  On the MI355X (largest over the cases of
a group; the four maps | per-tile sums | gradients, map form and fused | scalar loss):
    noise, every edge size      0.18 | 0.16 | 0.05 | 0.02        smooth      0.12 | 0.10 | 0.01 | 0.00
    tile counts 1..25           0.13 | 0.17 | 0.04 | 0.01        constant    0.06 | 0.01 | 0.00 | 0.01
    4099x3x5, 4095x3x5          0.16 | 0.18 | 0.08 | 0.01        dark        0.40 | 0.15 | 0.04 | 0.03
    64x33x699                   0.14 | 0.18 |  -   | 0.01        identical   0.14 | 0.02 | 0.01 | 0.00
    single bright pixel         0.64 | 0.11 | 0.06 | 0.06        zeros       0.64 | 0.13 | 0.00 | 0.06
    l1_mean value               0.11                             signed      0.15 | 0.13 | 0.04 | 0.02
The scalar against the float64 sum of the returned per-tile sums: at most 0.06 of its summation bound."""
import functools

import numpy as np
import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -1.5 * 2.0 ** 100
C1F, C2F = float(np.float32(R.C1)), float(np.float32(R.C2))          # what the kernels are given (float arguments)
LAM = float(np.float32(0.2))
UP = 1.75                                                             # non-unit upstream of the fused loss


class Guarded:
    """n floats of NaN between two guards"""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(float("nan"))

    def problems(self, name):
        out = []
        nan = torch.isnan(self.t)
        if bool(nan.any()):
            out.append(f"{name}: {int(nan.sum())} of {self.t.numel()} elements not written (first: {int(nan.nonzero()[0])})")
        if not bool((self.buf[:GUARD] == SENTINEL).all()) or not bool((self.buf[GUARD + self.t.numel():] == SENTINEL).all()):
            out.append(f"{name}: a guard was overwritten")
        return out


def _api():
    from diff_gaussian_rasterization import _C
    return _C, _C.lib()


def ssim_forward(x, y, want_dm):
    _C, lib = _api()
    P, H, W = x.shape
    outs = [Guarded(x.numel()) for _ in range(4 if want_dm else 1)]
    p = [_C.ptr(o.t) for o in outs] + [None] * (4 - len(outs))
    _C.check(lib.gsr_fused_ssim_forward(P, H, W, C1F, C2F, _C.ptr(x), _C.ptr(y), *p, _C._stream()))
    return outs


def ssim_backward(x, y, g, dm):
    _C, lib = _api()
    P, H, W = x.shape
    out = Guarded(x.numel())
    _C.check(lib.gsr_fused_ssim_backward(P, H, W, _C.ptr(x), _C.ptr(y), _C.ptr(g), *[_C.ptr(d) for d in dm], _C.ptr(out.t),
                                         _C._stream()))
    return out


def fused_forward(x, y, lam):
    _C, lib = _api()
    P, H, W = x.shape
    nblk = int(lib.gsr_fused_loss_blocks(P, H, W))
    dm = [Guarded(x.numel()) for _ in range(3)]
    partials, loss = Guarded(2 * nblk), Guarded(1)
    _C.check(lib.gsr_fused_l1_ssim_forward(P, H, W, C1F, C2F, lam, _C.ptr(x), _C.ptr(y), *[_C.ptr(d.t) for d in dm],
                                           _C.ptr(partials.t), _C.ptr(loss.t), _C._stream()))
    return dm, partials, loss


def fused_backward(x, y, lam, upstream, dm):
    _C, lib = _api()
    P, H, W = x.shape
    out = Guarded(x.numel())
    _C.check(lib.gsr_fused_l1_ssim_backward(P, H, W, lam, _C.ptr(x), _C.ptr(y), _C.ptr(upstream), *[_C.ptr(d) for d in dm],
                                            _C.ptr(out.t), _C._stream()))
    return out


def _worst(name, got, ref, bound, shape=None):
    """-> (largest error / bound, description of the first element outside its bound or None).  NaN counts as outside."""
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, float("inf")), ratio)
    bad = ~(err <= bound)
    msg = None
    if bool(bad.any()):
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        if shape is not None and len(idx) == 3:
            p, r, c = idx
            where = (f"plane {p} tile (y {r // R.TILE_H}, x {c // R.TILE_W}) at (row {r % R.TILE_H}, column {c % R.TILE_W}) "
                     f"= pixel ({r}, {c})")
        elif len(idx) == 2:
            gy, gx = R.tile_counts(*shape[1:])
            t = idx[0]
            where = f"tile {t} = plane {t // (gy * gx)} (y {(t % (gy * gx)) // gx}, x {t % gx}), {'ssim' if idx[1] == 0 else 'L1'} sum"
        else:
            where = str(idx)
        msg = (f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; worst {where}: got {float(got[idx])!r}, reference "
               f"{float(ref[idx])!r}, bound {float(bound[idx]):.3g}, error / bound {float(ratio[idx]):.3g}")
    return float(ratio.max()), msg


def run_case(label, kind, planes, H, W, spot=None, seed=0, backward=True):
    """every kernel of the SSIM family on one image pair; -> list of findings (empty: all is well)"""
    x64, y64 = R.make_pair(kind, planes, H, W, seed=seed, spot=spot)
    shape = (planes, H, W)
    gen = torch.Generator().manual_seed(7 + seed)
    g64 = torch.randn(shape, generator=gen, dtype=torch.float64).float().double() if backward else None
    ref = R.ssim_reference(x64, y64, g64, C1F, C2F)
    ref = R.fused_loss_reference(x64, y64, LAM, float(np.float32(UP)), C1F, C2F, ref=ref, grad=backward)
    x, y = x64.float().cuda(), y64.float().cuda()
    finds, ratios = [], {}

    def hold(name, got, key, bound_key=None):
        r, msg = _worst(name, got, ref[key], ref[bound_key or key + "_bound"], shape)
        ratios[name] = r
        if msg:
            finds.append(msg)

    # --- map form: forward with and without the saved maps, backward with a random upstream map ---
    outs = ssim_forward(x, y, True)
    only_map = ssim_forward(x, y, False)
    again = ssim_forward(x, y, True)
    for nm, o, o2 in zip(R.MAPS, outs, again):
        finds += o.problems(nm)
        hold(nm, o.t, nm)
        if not torch.equal(o.t, o2.t):
            finds.append(f"{nm}: two runs differ")
    finds += only_map[0].problems("ssim_map (forward without the saved maps)")
    if not torch.equal(only_map[0].t, outs[0].t):
        finds.append("ssim_map differs between the forward with and without the saved maps")
    dm = [o.t for o in outs[1:]]
    if backward:
        g = g64.float().cuda()
        grad, grad2 = ssim_backward(x, y, g, dm), ssim_backward(x, y, g, dm)
        finds += grad.problems("dL_dimg1")
        hold("dL_dimg1", grad.t, "grad")
        if not torch.equal(grad.t, grad2.t):
            finds.append("dL_dimg1: two runs differ")
    # --- fused form: saved maps, per-tile sums, scalar, backward with a device upstream ---
    fdm, partials, loss = fused_forward(x, y, LAM)
    fdm2, partials2, loss2 = fused_forward(x, y, LAM)
    for nm, o, o2, d in zip(R.MAPS[1:], fdm, fdm2, dm):
        finds += o.problems("fused " + nm)
        if not torch.equal(o.t, d):
            finds.append(f"fused {nm}: differs from the map form's (per-tile sums requested or not)")
        if not torch.equal(o.t, o2.t):
            finds.append(f"fused {nm}: two runs differ")
    finds += partials.problems("partials") + loss.problems("loss")
    if not (torch.equal(partials.t, partials2.t) and torch.equal(loss.t, loss2.t)):
        finds.append("partials / loss: two runs differ")
    hold("partials", partials.t.view(-1, 2), "partials")
    lv = float(loss.t[0])
    ratios["loss"] = abs(lv - ref["loss"]) / ref["loss_bound"]
    if not abs(lv - ref["loss"]) <= ref["loss_bound"]:
        finds.append(f"loss: got {lv!r}, reference {ref['loss']!r}, bound {ref['loss_bound']:.3g}")
    from_partials = float(R.loss_from_partials(partials.t.view(-1, 2).cpu(), LAM, x.numel()))
    sb = R.loss_summation_bound(partials.t.view(-1, 2).cpu(), LAM, x.numel())
    ratios["loss|partials"] = abs(lv - from_partials) / sb
    if not abs(lv - from_partials) <= sb:
        finds.append(f"loss: got {lv!r}, from the returned partials in float64 {from_partials!r}, summation bound {sb:.3g}")
    if backward:
        up = torch.tensor(UP, dtype=torch.float32, device="cuda")
        fg = fused_backward(x, y, LAM, up, [o.t for o in fdm])
        fg2 = fused_backward(x, y, LAM, up, [o.t for o in fdm])
        finds += fg.problems("fused dL_dimg1")
        hold("fused dL_dimg1", fg.t, "fused_grad")
        if not torch.equal(fg.t, fg2.t):
            finds.append("fused dL_dimg1: two runs differ")
    torch.cuda.synchronize()
    print(f"\n  {label}: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return finds


def _check(*a, **kw):
    finds = run_case(*a, **kw)
    assert not finds, "\n".join(finds)


# the tile is 32 wide and 16 high with a 5-pixel halo: sizes below the window, at and around the halo (5, 6, 10, 11), at and around
# one and two tiles, and widths / heights whose last tile holds less than a halo
SHAPES = [(1, 1), (5, 5), (6, 6), (16, 32), (17, 33), (33, 65), (1, 5), (5, 1), (1, 64), (32, 1), (6, 10), (11, 11), (11, 31),
          (15, 32), (16, 33), (16, 31), (17, 37), (21, 42), (21, 43), (26, 64), (27, 65), (32, 64), (33, 64), (32, 65), (27, 10),
          (5, 43), (15, 6), (26, 37), (33, 11), (6, 65), (32, 32), (11, 42)]


@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_noise_at_every_edge_size(H, W):
    planes = 1 + (H + W) % 3
    _check(f"noise {planes}x{H}x{W}", "noise", planes, H, W)


# n = planes x tiles around the strip walk's ceil(n / 8): once by planes of one tile, once by one or two planes of several tiles
TILE_COUNTS = [(1, 1, 9, 7)] + [(n, n, 6, 11) for n in (2, 7, 8, 9, 15, 16, 17, 23, 25)] + [
    (2, 1, 16, 33), (7, 1, 107, 20), (8, 2, 27, 43), (9, 1, 33, 65), (15, 1, 33, 151), (16, 2, 21, 100), (17, 1, 6, 534),
    (23, 1, 367, 5), (25, 1, 70, 150)]


@pytest.mark.parametrize("n,planes,H,W", TILE_COUNTS, ids=[f"n{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in TILE_COUNTS])
def test_tile_counts_around_the_strip_walk(n, planes, H, W):
    gy, gx = R.tile_counts(H, W)
    assert planes * gy * gx == n
    _check(f"n = {n}: {planes}x{H}x{W}", "noise", planes, H, W, seed=1)


# the forward walks two tiles per workgroup from 4096 tiles on.  4099 planes of one tile: ceil(4099 / 8) = 513 is odd, so every
# strip ends in a walk of one tile, the last strip is short and every walk crosses a plane; 64 x 3 x 22 = 4224 tiles: walks cross
# tile rows and planes inside bigger images; 4095 stays on the one-tile path beside them.
@pytest.mark.parametrize("planes,H,W,backward", [(4099, 3, 5, True), (4095, 3, 5, True), (64, 33, 699, False)])
def test_two_tiles_per_workgroup(planes, H, W, backward):
    _check(f"noise {planes}x{H}x{W}", "noise", planes, H, W, seed=2, backward=backward)


CLASS_SHAPES = [(2, 33, 65), (3, 17, 33), (1, 6, 6), (2, 26, 43)]


@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=["x".join(map(str, s)) for s in CLASS_SHAPES])
@pytest.mark.parametrize("kind", [k for k in R.CLASSES if k != "noise"])
def test_image_classes(kind, shape):
    _check(f"{kind} {'x'.join(map(str, shape))}", kind, *shape, seed=3)


@pytest.mark.parametrize("spot", [(15, 31), (16, 32), (0, 0), (32, 64)])
def test_single_bright_pixel(spot):
    """every pixel of the reference's moments is one window weight (or zero): a halo column or row read from the wrong place moves
    the weight under it"""
    x64, _ = R.make_pair("spot", 1, 33, 65, spot=spot)
    w = R.window2d()
    mu1 = R.conv(x64)[0]
    for dy in (-5, 0, 3, 5):
        for dx in (-5, -1, 0, 5):
            r, c = spot[0] + dy, spot[1] + dx
            if 0 <= r < 33 and 0 <= c < 65:
                assert float(mu1[r, c]) == float(w[5 - dy, 5 - dx])
    assert int((mu1 != 0).sum()) == (min(spot[0], 5) + 1 + min(32 - spot[0], 5)) * (min(spot[1], 5) + 1 + min(64 - spot[1], 5))
    _check(f"spot {spot}", "spot", 1, 33, 65, spot=spot)


@pytest.mark.parametrize("shape", [(3, 33, 65), (2, 17, 37)])
def test_python_entry_points_give_the_bits_of_the_direct_calls(shape):
    from diff_gaussian_rasterization._C import fusedssim, fusedssim_backward
    from fused_ssim import fused_ssim, fused_l1_ssim_loss
    x64, y64 = R.make_pair("noise", *shape, seed=4)
    x, y = x64.float().cuda(), y64.float().cuda()
    g = torch.randn(shape, generator=torch.Generator().manual_seed(5)).cuda()
    outs = ssim_forward(x, y, True)
    dm = [o.t.clone().view(shape) for o in outs[1:]]
    grad = ssim_backward(x, y, g, dm)
    # fusedssim / fusedssim_backward (C1, C2 arrive as Python floats and are rounded to float by the call)
    assert torch.equal(fusedssim(R.C1, R.C2, x, y).reshape(-1), outs[0].t)
    assert torch.equal(fusedssim_backward(R.C1, R.C2, x, y, g).reshape(-1), grad.t)
    assert torch.equal(fusedssim_backward(R.C1, R.C2, x, y, g, partials=tuple(dm)).reshape(-1), grad.t)
    # fused_ssim: the mean of the map; its backward hands the kernel the constant map 1 / N
    a = x.clone().requires_grad_(True)
    val = fused_ssim(a.unsqueeze(0), y.unsqueeze(0))
    val.backward()
    assert float(val.detach()) == float(outs[0].t.clone().view(1, *shape).mean())
    ones = torch.ones((), device="cuda").expand(1, *shape) / x.numel()
    assert torch.equal(a.grad.reshape(-1), ssim_backward(x, y, ones.contiguous().view(shape), dm).t)
    # fused_l1_ssim_loss with a non-unit upstream
    fdm, partials, loss = fused_forward(x, y, LAM)
    fg = fused_backward(x, y, LAM, torch.tensor(UP, dtype=torch.float32, device="cuda"), [o.t for o in fdm])
    a = x.clone().requires_grad_(True)
    val = fused_l1_ssim_loss(a, y, LAM)
    (UP * val).backward()
    assert float(val.detach()) == float(loss.t[0])
    assert torch.equal(a.grad.reshape(-1), fg.t)


# --------------------------------------------------------------------------------------------------------------------------
# weight * mean|(a - b) mask|
# --------------------------------------------------------------------------------------------------------------------------
L1_WEIGHT, L1_UP = float(np.float32(0.7)), 2.5
# the float4 body, the n & 3 tail, one / two / three / four workgroups (a workgroup takes 4 * 256 elements per trip), and one n
# behind 4 * 256 * 1024, where the grid is capped and a workgroup makes a second trip
L1_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 3 - 1, 4 * 256 * 3, 4 * 256 * 3 + 1, 4 * 256 * 1024 + 4 * 256 + 3]


@functools.lru_cache(maxsize=None)
def _l1_inputs(n):
    gen = torch.Generator().manual_seed(n)
    a = torch.rand(n, generator=gen)
    b = a + 0.05 * torch.randn(n, generator=gen)
    b[: max(1, n // 5)] = a[: max(1, n // 5)]                  # exact ties
    mask = (torch.rand(n, generator=gen) > 0.3).float() * (0.5 + torch.rand(n, generator=gen))
    return a, b, mask


def _l1_direct(a, b, mask):
    _C, lib = _api()
    n = a.numel()
    partials, out, grad = Guarded(int(lib.gsr_l1_mean_blocks())), Guarded(1), Guarded(n)
    partials.t.zero_()                                   # scratch: only the first blocks of it are written
    up = torch.tensor(L1_UP, dtype=torch.float32, device="cuda")
    _C.check(lib.gsr_l1_mean_forward(n, L1_WEIGHT, _C.ptr(a), _C.ptr(b), _C.ptr(mask), _C.ptr(partials.t), _C.ptr(out.t), _C._stream()))
    _C.check(lib.gsr_l1_mean_backward(n, L1_WEIGHT, _C.ptr(a), _C.ptr(b), _C.ptr(mask), _C.ptr(up), _C.ptr(grad.t), _C._stream()))
    finds = partials.problems("partials") + out.problems("out") + grad.problems("grad")
    assert not finds, "\n".join(finds)
    return out.t.clone(), grad.t.clone()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_mean_value_and_exact_gradient(n, masked):
    from fused_ssim import l1_mean_loss
    a, b, mask = _l1_inputs(n)
    mask = mask if masked else None
    ref, bound = R.l1_mean_reference(a.double(), b.double(), L1_WEIGHT, None if mask is None else mask.double())
    gref = R.l1_mean_grad_fp32(a.numpy(), b.numpy(), L1_WEIGHT, None if mask is None else mask.numpy(), L1_UP)
    da, db, dmask = a.cuda(), b.cuda(), None if mask is None else mask.cuda()
    out, grad = _l1_direct(da, db, dmask)
    out2, grad2 = _l1_direct(da, db, dmask)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    print(f"\n  n = {n}{' masked' if masked else ''}: error / bound {abs(float(out) - ref) / max(bound, 1e-300):.3f}")
    assert abs(float(out) - ref) <= bound, (float(out), ref, bound)
    assert np.array_equal(grad.cpu().numpy(), gref)                        # +-g m / n or 0, bit for bit (sign(0) = 0 included)
    # the Python entry point: the same bits
    x = da.clone().requires_grad_(True)
    val = l1_mean_loss(x, db, L1_WEIGHT, dmask)
    (L1_UP * val).backward()
    assert float(val.detach()) == float(out) and torch.equal(x.grad, grad)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", [5, 1025, 4 * 256 * 3 + 1])
def test_l1_mean_takes_views_that_start_inside_a_buffer(n, k):
    """gsr_l1_mean_forward reads float4s and refuses pointers that are not 16-byte aligned; buf[k:k+n] is contiguous, so
    `.contiguous()` does not move it: the wrapper copies such a view."""
    from fused_ssim import l1_mean_loss
    a, b, mask = _l1_inputs(n)
    res = []
    for off in (0, k):
        bufs = [torch.zeros(n + 8, device="cuda") for _ in range(3)]
        views = []
        for buf, src in zip(bufs, (a, b, mask)):
            buf[off:off + n] = src.cuda()
            views.append(buf[off:off + n])
        assert all(v.is_contiguous() and (v.data_ptr() & 15 != 0) == (off != 0) for v in views)
        x = views[0].detach().requires_grad_(True)
        val = l1_mean_loss(x, views[1], L1_WEIGHT, views[2])
        (L1_UP * val).backward()
        res.append((val.detach().clone(), x.grad.clone()))
    assert float(res[0][0]) == float(res[1][0]) and torch.equal(res[0][1], res[1][1])
    out, grad = _l1_direct(a.cuda(), b.cuda(), mask.cuda())
    assert float(res[1][0]) == float(out) and torch.equal(res[1][1], grad)
