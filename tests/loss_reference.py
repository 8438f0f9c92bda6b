"""Float64 reference of the loss kernels of csrc/ssim.hip, the per-pixel error bound they are held to, and two float32
restatements that show what float32 reaches.  Plain torch / numpy on the CPU; nothing here calls the HIP path.

  moments, maps_from_moments, ssim_reference      the five window moments (2-D window of oracle/loss_oracle.py: built and
                                                  normalised in float32, zero "same" padding), the map m and the three saved maps
                                                  dm_dmu1, dm_dsigma1_sq, dm_dsigma12 exactly as k_ssim_fwd defines them ("partials
                                                  holding E[xx], E[yy], E[xy] fixed"), the gradient
                                                  W*(g dm_dmu1) + 2x W*(g dm_dsigma1_sq) + y W*(g dm_dsigma12), and their bounds
  fused_loss_reference                            per-tile sums (32x16 tiles, (plane, y, x) order), scalar loss, gradient with the
                                                  (1-lambda)/n sign(x-y) term (sign(0) = 0), and their bounds
  ssim, training_loss                             the two scalars of oracle/loss_oracle.py (equal to it to 1e-13)
  l1_mean_reference, l1_mean_grad_fp32            weight * mean|(a-b) mask|: value + bound; the gradient bit for bit
  conv2d_fp32, separable_fp32                     the float32 restatements (the second one takes the mutations of
                                                  tests/test_loss_reference_cpu.py)
  make_pair                                       the image classes

Inputs are float32 values held in float64 (`t.float().double()`), so x - y and sign(x - y) are the same in both precisions.

THE BOUND.  u = 2^-24 (half an ulp, the relative error of one float32 rounding).  Every window moment v (mu1, mu2, E[xx], E[yy],
E[xy]) is given an uncertainty  dv = K u W*|terms of v|  (for non-negative images that is K u v); each map f(moments) gets
df = sum_v |df/dv| dv + 4 u |f|  with df/dv from autograd through the float64 element-wise formulas; the gradient gets |g| d(dm
maps) pushed through the same three convolutions with |x|, |y| in front, plus K u times the same expression on |g dm|.  No fixed
tolerance can do this job: sigma^2 = E[xx] - mu^2 sits over C2 = 9e-4, and on a flat image the float32 error of the map is 100x
what it is on noise.

K = 24 is the number of roundings on the longest path into one moment, between the float32 inputs and the float64 reference:
     1   the product that enters the horizontal pass: `s11 += w * a * a` is fma(fl(w * a), a, s11), fl(w * a) is rounded
    11   horizontal pass: the term of tap 0 goes through the rounding of all eleven FMAs of its accumulator
    11   vertical pass: the same for its eleven FMAs
     1   the reference's side: its 2-D window holds fl(g_i g_j), rounded to float32 once, the kernel multiplies by g_j and g_i
    --
    24   (mu1 and mu2 have no product to round: 23.  The backward's convolutions: fl(g dm) + 11 + 11 + 1 = 24.)
The roundings behind the moments (mu^2, the differences, A, B, C, D, the two v_rcp_f32 of 1 ulp, the products) are relative to
quantities no larger than the moments' own terms or to the result; the `4 u |f|` and the slack of a worst-case chain (only
the term of tap 0 sees all eleven roundings, and they do not all point the same way) carry them.  K is not tuned:
tests/test_loss_reference_cpu.py prints how much of the bound two float32 evaluations use and that deliberate defects exceed it.

Sums.  A per-tile sum is given the sum of its pixels' bounds plus L u sum|terms|, L the longest chain of additions in k_ssim_fwd:
  SSIM sum   2 (a thread adds its RPT = 2 pixels) + 6 (halving tree of a wave) + 2 ((w0 + w1) + (w2 + w3))          = 10
  L1 sum     1 (the rounding of x - y) + 4 (a thread adds its four pixels; 208 items, so one item per thread) + 6 + 2   = 13
k_loss_finalize: thread t adds tiles t, t + 1024, ...: ceil(nblk / 1024) additions, 6 for the wave's tree, 4 for the tree over the
sixteen wave sums (`finalize_chain`).  The scalar `(1 - l) (b inv_n) + l (1 - a inv_n)` then costs SCALAR_ROUNDINGS = 6 relative
to its two terms (inv_n: two products and a division; b inv_n or a inv_n; 1 - .; the product with l or 1 - l; the last addition is
relative to the result, which is smaller than the sum of the terms' magnitudes).
The fused backward forms its constants as g = -l inv_n up and g_l1 = (1 - l) inv_n up in float32: 3 roundings for inv_n, one
for 1 - l, one for each product: at most SCALAR_ROUNDINGS = 6 as well, added to K in front of the |g dm| expression and applied to
the L1 term (plus one for the addition of the L1 term to the rest).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
K = 24
C1 = 0.01 ** 2
C2 = 0.03 ** 2
TILE_W, TILE_H, RADIUS = 32, 16, 5
L_TILE_SSIM = 10
L_TILE_L1 = 13
SCALAR_ROUNDINGS = 6
FIN_THREADS = 1024


def finalize_chain(nblk):
    return -(-int(nblk) // FIN_THREADS) + 6 + 4


# ---------------------------------------------------------------------------------------------------------------------------
# window and convolution
# ---------------------------------------------------------------------------------------------------------------------------
def window1d():
    """float32 [11], as oracle/loss_oracle.py (and make_window() of ssim.hip) build it: float32 values, float32 normalisation"""
    g = torch.tensor([math.exp(-(x - RADIUS) ** 2 / float(2 * 1.5 ** 2)) for x in range(2 * RADIUS + 1)])
    return g / g.sum()


_w2 = {}


def window2d(dtype=torch.float64):
    """[11, 11]: the float32 outer product of the 1-D window (rounded to float32 once), held in `dtype`"""
    if dtype not in _w2:
        g = window1d().unsqueeze(1)
        _w2[dtype] = g.mm(g.t()).float().to(dtype).contiguous()
    return _w2[dtype]


def conv(x):
    """[planes, H, W] -> the same shape: 11x11 window, zero "same" padding, in x's dtype"""
    P = x.shape[0]
    if P > 16 and x.shape[1] * x.shape[2] <= 1024:                     # thousands of tiny planes: one channel, planes as the batch
        return F.conv2d(x.unsqueeze(1), window2d(x.dtype)[None, None], padding=RADIUS).squeeze(1)
    w =window2d(x.dtype)[None, None].expand(P, 1, -1, -1).contiguous()
    return F.conv2d(x.unsqueeze(0), w, padding=RADIUS, groups=P).squeeze(0)       # (the oracle's grouped form: the fastest in float64)


def moments(x, y):
    return conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)


def maps_from_moments(mu1, mu2, e11, e22, e12, c1=C1, c2=C2):
    """m, dm_dmu1, dm_dsigma1_sq, dm_dsigma12 per pixel (element-wise; any float dtype)"""
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, B = 2 * mu12 + c1, 2 * s12 + c2
    Cc, D = mu1_sq + mu2_sq + c1, s1 + s2 + c2
    inv = 1 / (Cc * D)
    m = A * B * inv
    d1 = 2 * mu2 * (B - A) * inv - m * 2 * mu1 / Cc + m * 2 * mu1 / D
    d2 = -m / D
    d3 = 2 * A * inv
    return m, d1, d2, d3


def backward_from_maps(x, y, g, d1, d2, d3):
    return conv(g * d1) + 2 * x * conv(g * d2) + y * conv(g * d3)


MAPS = ("ssim_map", "dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")


def ssim_reference(x, y, g=None, c1=C1, c2=C2, k=K):
    """x, y [planes, H, W] float64 (float32 values), g the upstream gradient of the map or None.
    -> dict: the four MAPS and `grad` (if g), each with its bound under "<name>_bound"."""
    assert x.dtype == torch.float64 and y.dtype == torch.float64 and x.dim() == 3
    mom = [v.detach().requires_grad_(True) for v in moments(x, y)]
    if bool((x >= 0).all()) and bool((y >= 0).all()):
        dmom = [k * U * v.detach() for v in mom]                     # the terms are non-negative: W*|terms| is the moment
    else:
        ax, ay = x.abs(), y.abs()
        dmom = [k * U * conv(ax), k * U * conv(ay), k * U * mom[2].detach(), k * U * mom[3].detach(), k * U * conv(ax * ay)]
    outs = maps_from_moments(*mom, c1, c2)
    res = {}
    for name, o in zip(MAPS, outs):
        part = torch.autograd.grad(o.sum(), mom, retain_graph=True, allow_unused=True)
        bd = 4 * U * o.detach().abs()
        for p, dv in zip(part, dmom):
            if p is not None:
                bd = bd + p.abs() * dv
        res[name] = o.detach()
        res[name + "_bound"] = bd
    if g is not None:
        d = [res[n] for n in MAPS[1:]]
        bd = [res[n + "_bound"] for n in MAPS[1:]]
        res["grad"] = backward_from_maps(x, y, g, *d)
        res["grad_bound"] = grad_bound(x, y, g, d, bd, k)
    return res


def grad_bound(x, y, g, d, bd, k=K):
    ga, ax, ay = g.abs(), x.abs(), y.abs()
    return (backward_from_maps(ax, ay, ga, *bd) + k * U * backward_from_maps(ax, ay, ga, *[v.abs() for v in d]))


# ---------------------------------------------------------------------------------------------------------------------------
# fused L1 + D-SSIM loss
# ---------------------------------------------------------------------------------------------------------------------------
def tile_counts(H, W):
    return -(-H // TILE_H), -(-W // TILE_W)


def tile_sums(v):
    """[planes, H, W] -> [planes * gy * gx] sums over 32x16 tiles in (plane, y, x) order"""
    P, H, W = v.shape
    gy, gx = tile_counts(H, W)
    pad = F.pad(v, (0, gx * TILE_W - W, 0, gy * TILE_H - H))
    return pad.reshape(P, gy, TILE_H, gx, TILE_W).sum(dim=(2, 4)).reshape(-1)


def loss_from_partials(partials, lam, n):
    """float64 scalar from [nblk, 2] (ssim sum, L1 sum)"""
    p = partials.double()
    return (1.0 - lam) * (p[:, 1].sum() / n) + lam * (1.0 - p[:, 0].sum() / n)


def loss_summation_bound(partials, lam, n):
    """what k_loss_finalize may add to the error of a scalar formed from `partials`: its summation chain and the scalar formula"""
    p = partials.double().abs()
    L = finalize_chain(p.shape[0])
    s, l1 = float(p[:, 0].sum()) / n, float(p[:, 1].sum()) / n
    return U * (L * (lam * s + (1.0 - lam) * l1) + SCALAR_ROUNDINGS * ((1.0 - lam) * l1 + lam * (1.0 + s)))


def fused_loss_reference(x, y, lam, upstream=1.0, c1=C1, c2=C2, k=K, ref=None, grad=True):
    """-> dict: partials [nblk, 2] + bound, loss + bound, fused_grad (of upstream * loss w.r.t. x; `grad`) + bound, and the maps
    of ssim_reference (`ref`: its result, if the caller has it).  `lam`, `upstream` are the float32 values the kernel is given,
    held in Python floats."""
    n = x.numel()
    g = torch.full_like(x, -lam / n * upstream)
    res = dict(ref) if ref is not None else ssim_reference(x, y, None, c1, c2, k)
    m, mb = res["ssim_map"], res["ssim_map_bound"]
    diff = (x - y).abs()
    res["partials"] = torch.stack([tile_sums(m), tile_sums(diff)], dim=1)
    res["partials_bound"] = torch.stack([tile_sums(mb) + L_TILE_SSIM * U * tile_sums(m.abs()), L_TILE_L1 * U * tile_sums(diff)], dim=1)
    res["loss"] = float(loss_from_partials(res["partials"], lam, n))
    res["loss_bound"] = (float((lam * res["partials_bound"][:, 0].sum() + (1.0 - lam) * res["partials_bound"][:, 1].sum()) / n)
                         + loss_summation_bound(res["partials"], lam, n))
    if not grad:
        return res
    d = [res[nm] for nm in MAPS[1:]]
    bd = [res[nm + "_bound"] for nm in MAPS[1:]]
    l1 = (1.0 - lam) / n * upstream * torch.sign(x - y)
    res["fused_grad"] = backward_from_maps(x, y, g, *d) + l1
    res["fused_grad_bound"] = (grad_bound(x, y, g, d, bd, k + SCALAR_ROUNDINGS) + (SCALAR_ROUNDINGS + 1) * U * l1.abs())
    return res


def ssim(img1, img2):
    """mean SSIM of [planes, H, W] (or [1, planes, H, W]) images: oracle/loss_oracle.ssim"""
    x, y = img1.reshape(-1, *img1.shape[-2:]), img2.reshape(-1, *img2.shape[-2:])
    return maps_from_moments(*moments(x, y))[0].mean()


def training_loss(image, gt, lam=0.2):
    return (1.0 - lam) * (image - gt).abs().mean() + lam * (1.0 - ssim(image, gt))


# ---------------------------------------------------------------------------------------------------------------------------
# weight * mean|(a - b) mask|
# ---------------------------------------------------------------------------------------------------------------------------
def l1_mean_chain(n, blocks_cap=1024):
    """longest chain of roundings into k_l1_partial / k_l1_finalize's result: x - y and the mask product (2), the four elements of
    a float4 as (. + .) + (. + .) (2), one addition per grid-stride trip, the tail element (1), the 256-thread LDS tree (8), the
    1024-thread tree of the finalize (10), weight / (float)n with (float)n itself and the last product (3)"""
    n4 = n // 4
    blocks = min(blocks_cap, max(1, -(-n4 // 256)))
    trips = -(-n4 // (blocks * 256)) if n4 else 0
    return 2 + 2 + trips + 1 + 8 + 10 + 3


def l1_mean_reference(a, b, weight, mask=None):
    """float64 value and its bound (every term is non-negative: sum|terms| is the value)"""
    d = (a - b) if mask is None else (a - b) * mask
    val = float(weight * d.abs().sum() / a.numel())
    return val, l1_mean_chain(a.numel()) * U * abs(val)


def l1_mean_grad_fp32(a, b, weight, mask, upstream):
    """k_l1_bwd bit for bit: g = fl(up * fl(weight / (float)n)); d = fl(fl(a - b) m); grad = g m, -g m or 0.  numpy float32."""
    f = np.float32
    a, b = a.astype(f), b.astype(f)
    m = np.ones_like(a) if mask is None else mask.astype(f)
    g = f(upstream) * (f(weight) / f(a.size))
    d = (a - b) * m
    gm = (g * m).astype(f)
    return np.where(d > 0, gm, np.where(d < 0, -gm, f(0))).astype(f)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 restatements
# ---------------------------------------------------------------------------------------------------------------------------
def conv2d_fp32(x, y, g=None, c1=C1, c2=C2):
    """the reference's own route in float32: 2-D conv2d of the moments, the element-wise formulas, the backward"""
    x, y = x.float(), y.float()
    outs = maps_from_moments(*moments(x, y), c1, c2)
    res = dict(zip(MAPS, outs))
    if g is not None:
        res["grad"] = backward_from_maps(x, y, g.float(), *outs[1:])
    return res


def _fma(a, b, c):
    # float32 operands: the product is exact in float64; one float64 rounding of the sum in front of the float32 one
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _pass(v, w, axis):
    """11-tap FMA accumulation from tap 0 along `axis` of [planes, H, W] float32, zero padding"""
    pad = [(0, 0)] * 3
    pad[axis] = (RADIUS, RADIUS)
    p = np.pad(v, pad)
    n = v.shape[axis]
    acc = np.zeros_like(v)
    for t in range(2 * RADIUS + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(t, t + n)
        acc = _fma(np.broadcast_to(w[t], v.shape), p[tuple(sl)], acc)
    return acc


def separable_fp32(x, y, g=None, c1=C1, c2=C2, lam=None, mutate=None):
    """numpy float32 in k_ssim_fwd / k_ssim_bwd's order: horizontal pass, then vertical, FMA accumulation from tap 0,
    fl(w a) in front of the second moments' FMAs, v_rcp_f32 replaced by a division; per-tile sums by float64 addition of the
    float32 pixels (the summation order is not what this restatement is about).
    mutate: None | "tap" (outer tap of the horizontal window dropped) | "seam" (the left halo of the tiles at x0 = 32 read one
    column to the left) | "rows" (the tile's L1 sum taken from memory without the gy < H mask: row gy >= H of a plane is row gy - H
    of the next plane, nothing behind the last) | "window64" (window normalised in float64, then rounded)."""
    f = np.float32
    x, y = x.numpy().astype(f), y.numpy().astype(f)
    if mutate == "window64":
        v = np.array([math.exp(-(i - RADIUS) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
        w = (v / v.sum()).astype(f)
    else:
        w = window1d().numpy().astype(f)
    wh = w.copy()
    if mutate == "tap":
        wh[0] = 0
    P, H, W = x.shape

    def horizontal(v, shifted):
        out = _pass(v, wh, 2)
        if mutate == "seam" and W > TILE_W + RADIUS:
            # outputs 32..36 are the ones of the tile at x0 = 32 that read its left halo (columns 27..31): taken from 26..30
            out[:, :, TILE_W:TILE_W + RADIUS] = _pass(shifted, wh, 2)[:, :, TILE_W:TILE_W + RADIUS]
        return out

    def shift(v):
        s = v.copy()
        s[:, :, TILE_W - RADIUS:TILE_W] = v[:, :, TILE_W - RADIUS - 1:TILE_W - 1]
        return s

    def sep(v, vs=None):
        return _pass(horizontal(v, vs), w, 1)

    def second(a, b):                    # sum_k fma(fl(w a), b, acc) horizontally, plain FMA vertically
        def hpass(a, b):
            pa, pb = np.pad(a, [(0, 0), (0, 0), (RADIUS, RADIUS)]), np.pad(b, [(0, 0), (0, 0), (RADIUS, RADIUS)])
            acc = np.zeros_like(a)
            for t in range(11):
                acc = _fma((wh[t] * pa[:, :, t:t + W]).astype(f), pb[:, :, t:t + W], acc)
            return acc
        out = hpass(a, b)
        if mutate == "seam" and W > TILE_W + RADIUS:
            out[:, :, TILE_W:TILE_W + RADIUS] = hpass(shift(a), shift(b))[:, :, TILE_W:TILE_W + RADIUS]
        return _pass(out, w, 1)

    mu1, mu2 = sep(x, shift(x)), sep(y, shift(y))
    e11, e22, e12 = second(x, x), second(y, y), second(x, y)
    c1, c2 = f(c1), f(c2)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, B = f(2) * mu12 + c1, f(2) * s12 + c2
    Cc, D = mu1_sq + mu2_sq + c1, s1 + s2 + c2
    rCc, rD = f(1) / Cc, f(1) / D
    inv = rCc * rD
    m = A * B * inv
    d1 = f(2) * mu2 * (B - A) * inv - m * f(2) * mu1 * rCc + m * f(2) * mu1 * rD
    d2 = -m * rD
    d3 = f(2) * A * inv
    res = dict(zip(MAPS, (torch.from_numpy(v) for v in (m, d1, d2, d3))))
    if g is not None:
        g = g.numpy().astype(f)
        t = [sep(g * d, shift(g * d)) for d in (d1, d2, d3)]
        res["grad"] = torch.from_numpy(t[0] + f(2) * x * t[1] + y * t[2])
    if lam is not None:
        diff = np.abs(x - y).astype(np.float64)
        l1 = tile_sums(torch.from_numpy(diff))
        if mutate == "rows":
            gy, gx = tile_counts(H, W)
            flat = np.concatenate([diff.reshape(-1, W), np.zeros((gy * TILE_H, W))])        # rows behind the last plane: nothing
            rows = (np.arange(P)[:, None] * H + np.arange(gy * TILE_H)[None, :]).reshape(-1)
            l1 = tile_sums(torch.from_numpy(flat[rows].reshape(P, gy * TILE_H, W)))
        res["partials"] = torch.stack([tile_sums(torch.from_numpy(m.astype(np.float64))), l1], dim=1)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# image classes
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = ("noise", "smooth", "constant", "dark", "identical", "zeros", "signed")


def make_pair(kind, planes, H, W, seed=0, spot=None):
    """-> (x, y) float64 [planes, H, W] holding float32 values.  kind: one of CLASSES, or "spot" (one bright pixel at `spot` =
    (row, column) of plane 0 in x, half as bright in y, zeros elsewhere)."""
    gen = torch.Generator().manual_seed(1000003 * seed + 8191 * planes + 131 * H + W)
    a = torch.rand(planes, H, W, generator=gen, dtype=torch.float64)
    b = (a + 0.1 * torch.randn(planes, H, W, generator=gen, dtype=torch.float64)).clamp(0, 1)
    yy = torch.linspace(0, 1, H, dtype=torch.float64).view(1, H, 1)
    xx = torch.linspace(0, 1, W, dtype=torch.float64).view(1, 1, W)
    if kind == "noise":
        x, y = a, b
    elif kind == "smooth":
        x = (0.2 + 0.6 * xx * yy).expand(planes, H, W).clone()
        y = (x + 0.01 * torch.sin(7 * xx)).clamp(0, 1)
    elif kind == "constant":
        x, y = torch.full_like(a, 0.70), torch.full_like(a, 0.69)
    elif kind == "dark":
        x, y = 0.02 * a, 0.02 * b
    elif kind == "identical":
        x, y = a, a.clone()
    elif kind == "zeros":
        x, y = torch.zeros_like(a), torch.zeros_like(a)
    elif kind == "signed":
        x = 2.0 * a - 0.5
        y = x + 0.1 * torch.randn(planes, H, W, generator=gen, dtype=torch.float64)
    elif kind == "spot":
        x, y = torch.zeros_like(a), torch.zeros_like(a)
        x[0, spot[0], spot[1]] = 1.0
        y[0, spot[0], spot[1]] = 0.5
    else:
        raise ValueError(kind)
    return x.float().double(), y.float().double()
