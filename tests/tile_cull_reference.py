"""float64 reconstruction of the per-tile depth cut-offs the compositing forward learns (csrc/render.hip k_render_fwd, the block
behind the COUNT return; include/gsr.h gsr_forward_async_culled).  numpy only, no GPU, and nothing imported from the library:
the rules are restated here.

Input is one frame as the debug views expose it: the per-Gaussian records ([P, 12]: mean x, mean y, A', B', C', opacity, ... with
log2(alpha / opacity) = (A' dx + B' dy) dx + C' dy dy, d = mean - pixel; gsr_common.h), the per-tile ranges, the sorted point
list and the UNSORTED per-Gaussian depth keys.  Every pixel of every tile is composited again in float64 with the published rules:

    power > 0                         -> skip
    alpha = min(0.99, o e^power)      (e^power = 2^(log2 form))
    alpha < 1/255                     -> skip
    test_T = T (1 - alpha) < 1e-4     -> the pixel stops AT this entry (which is not blended); else T = test_T

    stop_at  = 1-based list position of the stopping entry, 0 if the pixel never saturated
    need     = max over the tile's pixels inside the image; all ones if one of them never saturated
    k        = ((need q8) >> 8) + add                       (need not all ones)
    cut-off  = depth key of the Gaussian at 0-based list index k if k < len, all ones otherwise (untruncated frame)

Ambiguous tiles.  The kernel composites in float32: T over a few hundred entries is off by about n 6e-8 <= 1e-5 relative, exp2 by
about 1e-6.  A comparison is DOUBTFUL if it lies within BAND = 1e-4 relative (ten times that error) of its threshold:
    alpha against 1/255      |255 alpha - 1|      <= BAND
    power against 0          |power|              <= BAND (|A' dx dx| + |B' dx dy| + |C' dy dy|), unless all three terms are zero
                             (dx = dy = 0: power is exactly 0 on both sides); 0 has no scale of its own, the rounding error of
                             the form is relative to the magnitude of its terms
    test_T against 1e-4      |test_T / 1e-4 - 1|  <= BAND
A tile is AMBIGUOUS - left out of exact comparisons, and counted - if a doubtful comparison at or before a stop DECIDES its `need`.
Nearly every tile of a real frame has some doubtful alpha >= 1/255 test among its ~256 x need comparisons (the 1/255 contour of
every splat runs between some pair of pixels; 28 % and 67 % of the tiles of the first two cases below), and almost none of them
moves the tile's maximum.  So the doubt is followed through instead: with every doubtful skip test taken as "blend" the pixel's T
is as small as it can be and it stops as EARLY as it can (first entry with test_T < 1e-4 (1 + BAND)); with every one taken as
"skip", as LATE as it can (first surely-blended entry with test_T < 1e-4 (1 - BAND); never, if there is none).  Whatever the
float32 kernel decided, each pixel's stop lies between the two, and so does the tile's need between the maxima of the two.  The
tile is ambiguous iff those maxima differ; where they agree, need is known exactly and is compared exactly.
A case may leave out at most AMBIGUOUS_CAP of its tiles."""
import math

import numpy as np

TILE = 16
ALL = 0xFFFFFFFF              # cut-off "no limit", need "a pixel never saturated"
NO_ID = 0xFFFFFFFF            # padding slot of a list: never blended
BAND = 1.0e-4
AMBIGUOUS_CAP = 0.02
MARGIN_Q8, MARGIN_ADD = 448, 48          # the launcher's defaults: 1.75 x + 48
LOG2E = 1.4426950408889634

# The frames of tests/test_tile_cull_cutoffs_gpu.py (a) and (c): name -> P, make_gaussians seed and scale, camera seed, W, H.
# Seeds chosen by running this module on the oracle's float64 records and lists (tests/test_tile_cull_reference_cpu.py keeps
# asserting it): at most AMBIGUOUS_CAP of the tiles of every case are ambiguous.
CASES = {
    "saturating": dict(P=4000, seed=151, scale=2.5, cam_seed=152, W=192, H=128),
    "sparse": dict(P=4000, seed=151, scale=0.7, cam_seed=152, W=192, H=128),
    "partial_tiles": dict(P=3000, seed=161, scale=2.0, cam_seed=162, W=200, H=120),
    "single_tile": dict(P=600, seed=171, scale=2.0, cam_seed=172, W=16, H=16),
    "small": dict(P=1000, seed=181, scale=2.0, cam_seed=182, W=40, H=24),
    "three": dict(P=3, seed=191, scale=6.0, cam_seed=192, W=64, H=48),
}


def tile_grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def records_from_oracle(pre):
    """oracle.gs_oracle.Preprocessed (float64) -> (rec [P, 12] float64 in the kernel's layout, depth keys [P] uint32)."""
    P = pre.xy.shape[0]
    rec = np.zeros((P, 12), dtype=np.float64)
    con = pre.conic.detach().numpy().astype(np.float64)
    rec[:, 0:2] = pre.xy.detach().numpy()
    rec[:, 2] = -0.5 * LOG2E * con[:, 0]
    rec[:, 3] = -LOG2E * con[:, 1]
    rec[:, 4] = -0.5 * LOG2E * con[:, 2]
    rec[:, 5] = pre.opacity.detach().numpy()
    keys = pre.depths.detach().numpy().astype(np.float32).view(np.uint32).copy()
    return rec, keys


def composite_tile(rec, ids, x0, y0, W, H):
    """One tile's list against its inside pixels.  -> (need, ambiguous, stop_at [pixels])"""
    xs = np.arange(x0, min(x0 + TILE, W), dtype=np.float64)
    ys = np.arange(y0, min(y0 + TILE, H), dtype=np.float64)
    px = np.tile(xs, len(ys))
    py = np.repeat(ys, len(xs))
    n = len(ids)
    if n == 0:
        return ALL, False, np.zeros(px.size, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    # (a prefix of the list is the whole answer once every pixel has surely stopped inside it: all stops are first occurrences)
    m = 256
    while True:
        need, ambiguous, stop_at, settled = _composite_prefix(rec, ids[:m], px, py)
        if settled or m >= n:
            return need, ambiguous, stop_at
        m *= 4


def _composite_prefix(rec, ids, px, py):
    n = len(ids)
    real = (ids != NO_ID)[:, None]
    r = np.asarray(rec, dtype=np.float64)[np.where(ids != NO_ID, ids, 0)]
    dx = r[:, 0:1] - px[None, :]
    dy = r[:, 1:2] - py[None, :]
    A, B, Cc, op = r[:, 2:3], r[:, 3:4], r[:, 4:5], r[:, 5:6]
    power = (A * dx + B * dy) * dx + Cc * dy * dy
    mag = np.abs(A) * dx * dx + np.abs(B * dx * dy) + np.abs(Cc) * dy * dy
    with np.errstate(over="ignore", under="ignore"):
        alpha = np.minimum(0.99, op * np.exp2(np.minimum(power, 64.0)))
    ok = real & (power <= 0.0) & (alpha >= 1.0 / 255.0)
    T_incl = np.cumprod(np.where(ok, 1.0 - alpha, 1.0), axis=0)      # = test_T of every entry up to the first stop
    stop = ok & (T_incl < 1.0e-4)
    stopped = stop.any(axis=0)
    first = np.argmax(stop, axis=0)
    stop_at = np.where(stopped, first + 1, 0).astype(np.int64)
    need = ALL if not stopped.all() else int(stop_at.max())
    # which comparisons lie inside the band, and the earliest / latest entry each pixel can stop at if they fall either way
    near_power = (mag > 0.0) & (np.abs(power) <= BAND * mag)
    near_alpha = np.abs(255.0 * alpha - 1.0) <= BAND
    surely = ok & ~near_power & ~near_alpha
    maybe = real & ((power <= 0.0) | near_power) & ((alpha >= 1.0 / 255.0) | near_alpha)
    T_low = np.cumprod(np.where(maybe, 1.0 - alpha, 1.0), axis=0)        # every doubtful entry blended: T as small as it can be
    T_high = np.cumprod(np.where(surely, 1.0 - alpha, 1.0), axis=0)      # none of them blended
    early = maybe & (T_low < 1.0e-4 * (1.0 + BAND))
    late = surely & (T_high < 1.0e-4 * (1.0 - BAND))
    never = n + 1                                                        # (orders behind every list position)
    earliest = np.where(early.any(axis=0), np.argmax(early, axis=0) + 1, never)
    latest = np.where(late.any(axis=0), np.argmax(late, axis=0) + 1, never)
    assert (earliest <= np.where(stopped, stop_at, never)).all() and (np.where(stopped, stop_at, never) <= latest).all()
    ambiguous = bool(earliest.max() != latest.max())
    return need, ambiguous, stop_at, bool((latest < never).all())


def expected_cutoffs(rec, ranges, point_list, depth_keys, W, H, q8=MARGIN_Q8, add=MARGIN_ADD):
    """-> dict of per-tile arrays: need (uint32; ALL = a pixel never saturated), k (int64; -1 where need is ALL), len (int64),
    cutoff (uint32: what an UNTRUNCATED frame leaves), ambiguous (bool)."""
    gx, gy = tile_grid(W, H)
    tiles = gx * gy
    ranges = np.asarray(ranges).astype(np.int64).reshape(tiles, 2)
    point_list = np.asarray(point_list).astype(np.int64)
    depth_keys = np.asarray(depth_keys).astype(np.int64)
    need = np.zeros(tiles, dtype=np.uint32)
    k = np.full(tiles, -1, dtype=np.int64)
    length = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    cutoff = np.full(tiles, ALL, dtype=np.uint32)
    ambiguous = np.zeros(tiles, dtype=bool)
    for t in range(tiles):
        ty, tx = divmod(t, gx)
        lo, hi = int(ranges[t, 0]), int(ranges[t, 1])
        nd, ambiguous[t], _ = composite_tile(rec, point_list[lo:hi], tx * TILE, ty * TILE, W, H)
        need[t] = nd
        if nd == ALL:
            continue
        k[t] = ((nd * int(q8)) >> 8) + int(add)
        if k[t] < length[t]:
            g = int(point_list[lo + k[t]])
            cutoff[t] = depth_keys[g] if g != NO_ID else ALL
    return dict(need=need, k=k, len=length, cutoff=cutoff, ambiguous=ambiguous)


def case_scene(name):
    """-> (RawGaussians, camera, sh degree, W, H) of CASES[name]"""
    from scene_utils import make_gaussians, fibonacci_cameras
    c = CASES[name]
    raw = make_gaussians(c["P"], 1, seed=c["seed"], scale_factor=c["scale"])
    cam = fibonacci_cameras(2, c["W"], c["H"], seed=c["cam_seed"])[0]
    return raw, cam, 1, c["W"], c["H"]


def stack_scene(n, opacity=0.8, spread=40.0, gap=0.05):
    """A depth-ordered stack of `n` identical wide splats in front of a 16 x 16 camera: isotropic, `spread` pixels wide at the
    first one, centred on pixel (7.5 + 0.5, ...) = the optical axis, `gap` apart in depth.  -> (RawGaussians, camera, 0, 16, 16)"""
    import torch
    from scene_utils import look_at_camera
    from scene_utils.synthetic import RawGaussians, SH_C0
    W = H = 16
    fovx = 0.6911
    cam = look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), fovx, W, H)
    focal = W / (2.0 * math.tan(0.5 * fovx))
    z = 4.0 + gap * torch.arange(n, dtype=torch.float32)
    xyz = torch.stack([torch.zeros(n), torch.zeros(n), z - 4.0], dim=1)
    sigma = spread * 4.0 / focal                                          # world units: `spread` pixels at depth 4
    scaling = torch.full((n, 3), math.log(sigma))
    rotation = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1)
    logit = math.log(opacity / (1.0 - opacity))
    f_dc = torch.full((n, 1, 3), (0.6 - 0.5) / SH_C0)
    raw = RawGaussians(xyz, f_dc, torch.zeros(n, 0, 3), scaling, rotation, torch.full((n, 1), logit), 0)
    return raw, cam, 0, W, H


def oracle_frame(raw, cam, deg, W, H):
    """The oracle's own float64 records and lists of a scene (no compositing).  -> (rec, ranges, point_list, depth_keys)"""
    import torch
    from oracle import gs_oracle as O
    from helpers import leaf_inputs, settings_for
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    s = settings_for(cam, deg, torch.zeros(3))
    with torch.no_grad():
        pre = O.preprocess(inp["means3D"], None, inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                           rotations=inp["rotations"])
        point_list, ranges, _ = O.bin_instances(pre, W, H)
    rec, keys = records_from_oracle(pre)
    return rec, ranges.numpy(), point_list.numpy(), keys
