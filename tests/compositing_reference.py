"""float64 replay of the compositing kernels on a frame's own records (csrc/render.hip: k_render_fwd, k_render_bwd, k_render_bwd_tile,
k_render_bwd_tile_mx).  numpy only, no GPU, nothing imported from the library: the rules are restated here, on top of what
tests/tile_cull_reference.py already states (record layout, scenes, the oracle's frame).

Input is one frame as the debug views expose it: rec [P, 12] = (mean x, mean y, A', B') (C', opacity, cut-off, r) (g, b, depth plane
value, depth) with log2(alpha / opacity) = (A' dx + B' dy) dx + C' dy dy, d = mean - pixel; the per-tile ranges; the sorted list.

FORWARD, per pixel inside the image, front to back over the tile's list:
    power > 0                              -> skip
    alpha = min(0.99, o 2^power)
    alpha < 1/255                          -> skip
    test_T = T (1 - alpha) < 1e-4          -> the pixel stops AT this entry (which is not blended); else w = alpha T, T = test_T
    colour_c = sum w c_c + T_final bg_c,  depth plane = sum w v  (v = word 10 of the record: 1/depth or depth, whichever the
    projection stored), final_T, n_contrib = 1-based position of the last blended entry (0: none), alpha plane = 1 - final_T.

BACKWARD, per (tile, list position): entries 1 .. n_contrib of every pixel back to front, n_contrib and final_T TAKEN FROM THE FRAME'S
IMAGE STATE (the kernels read them from there).  With gp = dL/dcolour, gd = dL/d(depth plane), gA = dL/d(alpha plane) of the pixel,
nTb = -final_T (bg . gp - gA), T = final_T, S = 0, for each entry that passes the two skip tests:
    T <- T / (1 - alpha);  dch = alpha T;  cg = c . gp + v gd;  diff = cg - S;  S <- S + alpha diff
    h = G (diff T + nTb / (1 - alpha)),  G = 2^power                            (= dL/dopacity_eff of this pixel and entry)
    record = sum over the tile's pixels of (h dx, h dy, h dx^2, h dx dy, h dy^2, h, dch gp_r, dch gp_g, dch gp_b, dch gd)
The records of one Gaussian are summed in slot order (k_preprocess_bwd) and dL/dmean2D = (W/2, H/2) o (-cA M0 - cB M1,
-cC M1 - cB M0) with the conic (cA, cB, cC) = (-2 A', -B', -2 C') / log2(e) and M0, M1 the summed first two values.

SCALE.  Every output comes with S = the float64 sum of the ABSOLUTE values of its terms, taken all the way down: |c| w and |bg| T
for a colour; for a record value, the pixel's term with every difference replaced by the sum of the magnitudes of its operands
(|h| <= G ((|c . gp| terms + the same recurrence on magnitudes) T + final_T (|bg gp| terms + |gA|) / (1 - alpha))).  A product has one
term: final_T is measured relative to itself, the alpha plane to 1 + final_T.  Errors are |got - ref| / S: no conditioning in them.

Each replay exists in float64 (the reference) and in plain float32 numpy, sequential, every operation rounded on its own (the
YARDSTICK: the bound of a value class is 4 x the largest error figure of the float32 replay over all cases, floor 2^-24; it is not
what a kernel is compared with).  Both use the kernels' float32 constants (1.0f / 255.0f, 0.99f, 0.0001f) unless published = True.

DOUBT.  A test near its threshold can fall either way in float32.  With u = 2^-24 and mag = |A' dx dx| + |B' dx dy| + |C' dy dy|:
    power:  dx and dy carry one rounding each (u relative), A' dx one, the inner sum one, the final sum one, in either evaluation
            order (fused or not): |error| <= 6 u mag, taken as 8 u mag.
    alpha:  exp2 within one ulp (2 u) on the hardware and in numpy, the product with the opacity u, and ln 2 x the error of power:
            relative error <= ln 2 x 8 u mag + 4 u.
    T:      per blended entry one rounding for 1 - alpha and one for the product (2 u) and alpha / (1 - alpha) x the relative
            error of alpha (nothing from alpha when it is capped: 1 - 0.99f is the same number everywhere); the bound is the sum
            over the entries blended so far.
The band of each test is SAFETY = 2 x that first-order bound (typically 1e-6 .. 2e-5 for alpha, where tile_cull_reference.py takes
a flat 1e-4, and up to ~2e-4 for a stop after a few hundred entries).  A (pixel, entry) pair is DOUBTFUL if one of its tests lies
inside its band while the other one does not already decide it, and the pixel can still be alive there.  Doubt is followed through,
not excluded: a tile with d <= MAX_DOUBT = 3 doubtful pairs is replayed under each of the 2^d assignments and a kernel passes on
that tile if one assignment matches all of the tile's outputs.  In the forward the pixels are independent, so the assignments are
tried per pixel (every new near-threshold stop test that an assignment brings up joins the set); in the backward the stop test
does not exist (n_contrib is given) and a record sums all pixels, so the product over the tile's doubtful pairs is tried.  Tiles with
d > 3 are LEFT OUT, counted and reported; a case may leave out at most LEFT_OUT_CAP = 2 % of its tiles."""
import itertools
import math

import numpy as np

import tile_cull_reference as R

TILE = R.TILE
NO_ID = R.NO_ID
LOG2E = R.LOG2E
U = 2.0 ** -24
FLOOR = U                      # one float32 rounding: no bound is tighter
FACTOR = 4.0                   # a different but fixed summation order, the hardware's exp2 against numpy's
SAFETY = 2.0
MAX_DOUBT = 3
PREFIX = 256                   # list entries the forward replays look at first (x 4 until every pixel has stopped)
LEFT_OUT_CAP = 0.02
RECORD_VALUES = ("h_dx", "h_dy", "h_dx2", "h_dxdy", "h_dy2", "h", "d_r", "d_g", "d_b", "d_depth")
FORWARD_CLASSES = ("color", "depth", "final_T", "alpha")
CLASSES = FORWARD_CLASSES + RECORD_VALUES + ("mean2D",)
STACK_OPACITY_A = 0.012
STACK_A_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)

# name -> P, SH degree, make_gaussians seed and scale, per-axis log-scale spread (and its seed), camera (seed, count, index), W, H,
# background.  Seeds chosen by running this module on the oracle's records (tests/test_compositing_reference_cpu.py keeps asserting
# it): at most LEFT_OUT_CAP of the tiles of every case are left out.  "regular" and "needles" are the scenes of
# tests/sweeps/mx_vs_swap_error.py.
CASES = {
    "regular": dict(P=6000, deg=2, seed=401, scale=0.8, spread=0.0, cam=(403, 3, 2), W=208, H=144, bg=(0.3, 0.2, 0.1)),
    "saturating": dict(P=4000, deg=1, seed=151, scale=2.5, spread=0.0, cam=(152, 2, 0), W=192, H=128, bg=(0.0, 0.0, 0.0)),
    "sparse": dict(P=4000, deg=1, seed=151, scale=0.7, spread=0.0, cam=(152, 2, 0), W=192, H=128, bg=(0.0, 0.0, 0.0)),
    "partial_tiles": dict(P=3000, deg=1, seed=161, scale=2.0, spread=0.0, cam=(162, 2, 0), W=200, H=120, bg=(0.7, 0.1, 0.4)),
    "single_tile": dict(P=600, deg=1, seed=171, scale=2.0, spread=0.0, cam=(172, 2, 0), W=16, H=16, bg=(0.0, 0.0, 0.0)),
    "needles": dict(P=6000, deg=2, seed=401, scale=0.8, spread=1.3, spread_seed=402, cam=(403, 3, 2), W=208, H=144,
                    bg=(0.3, 0.2, 0.1)),
    "needles_08": dict(P=6000, deg=2, seed=411, scale=0.8, spread=0.8, spread_seed=412, cam=(413, 3, 1), W=208, H=144,
                       bg=(0.0, 0.0, 0.0)),
}
# The float32 replay's largest |got - float64 replay| / S over all cases (yardstick(); the case it comes from), per value class:
# what the bounds of tests/test_compositing_replay_gpu.py are derived from.  The anisotropic scenes set most of them: there the
# terms of the power form are hundreds of times larger than the power itself, and float32 evaluates it to u x their magnitude.
YARDSTICK = {
    "color": 4.5518e-05,   # needles
    "depth": 1.0339e-06,   # stack_a_513
    "final_T": 1.7128e-04,   # needles
    "alpha": 2.8867e-07,   # stack_a_65
    "h_dx": 1.5916e-05,   # needles_08
    "h_dy": 1.5871e-05,   # needles_08
    "h_dx2": 1.5905e-05,   # needles_08
    "h_dxdy": 1.5931e-05,   # needles_08
    "h_dy2": 1.5888e-05,   # needles_08
    "h": 1.5901e-05,   # needles_08
    "d_r": 2.2543e-05,   # needles_08
    "d_g": 3.2880e-05,   # needles
    "d_b": 2.4262e-05,   # needles
    "d_depth": 2.4177e-05,   # needles
    "mean2D": 2.5884e-07,   # partial_tiles
}

# (b) stacks whose pixels stop on both sides of a batch end k: name -> n, opacity, k
STACK_B = {"stop_64": dict(n=80, opacity=0.138, k=64), "stop_128": dict(n=150, opacity=0.0705, k=128),
           "stop_256": dict(n=330, opacity=0.040, k=256)}


def case_scene(name):
    """-> (RawGaussians, camera, sh degree, W, H, bg [3] float32) of CASES[name] / "stack_a_<n>" / STACK_B[name]"""
    if name.startswith("stack_a_"):
        # (gap 0.002: the deepest of 513 splats is still 32 pixels wide, alpha >= 0.011 in the tile's corners)
        return R.stack_scene(int(name[8:]), opacity=STACK_OPACITY_A, gap=0.002) + (np.array([0.2, 0.5, 0.7], dtype=np.float32),)
    if name in STACK_B:
        c = STACK_B[name]
        return R.stack_scene(c["n"], opacity=c["opacity"]) + (np.array([0.2, 0.5, 0.7], dtype=np.float32),)
    import torch
    from scene_utils import make_gaussians, fibonacci_cameras
    c = CASES[name]
    raw = make_gaussians(c["P"], c["deg"], seed=c["seed"], scale_factor=c["scale"])
    if c["spread"]:
        gen = torch.Generator().manual_seed(c["spread_seed"])
        raw.scaling = raw.scaling + c["spread"] * torch.randn(raw.scaling.shape, generator=gen)
    seed, count, index = c["cam"]
    cam = fibonacci_cameras(count, c["W"], c["H"], seed=seed)[index]
    return raw, cam, c["deg"], c["W"], c["H"], np.array(c["bg"], dtype=np.float32)


def all_case_names():
    return list(CASES) + [f"stack_a_{n}" for n in STACK_A_SIZES] + list(STACK_B)


def upstream(W, H, seed=3):
    """The gradients every backward of a case is given: dL/dcolour [3, H, W], dL/d(depth plane) [H, W], dL/d(alpha plane) [H, W]"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32),
            rng.standard_normal((H, W)).astype(np.float32))


def oracle_frame(raw, cam, deg, W, H, depth_z=False):
    """tile_cull_reference.oracle_frame with the colour, depth-plane and depth words of the records filled in.
    -> (rec [P, 12] float64, ranges, point_list, oracle Preprocessed)"""
    import torch
    from oracle import gs_oracle as O
    from helpers import leaf_inputs, settings_for
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    s = settings_for(cam, deg, torch.zeros(3))
    with torch.no_grad():
        pre = O.preprocess(inp["means3D"], None, inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                           rotations=inp["rotations"])
        point_list, ranges, _ = O.bin_instances(pre, W, H)
    rec, _ = R.records_from_oracle(pre)
    z = pre.depths.numpy().astype(np.float64)
    zs = np.where(pre.radii.numpy() > 0, z, 1.0)
    rec[:, 7] = pre.rgb.numpy()[:, 0]
    rec[:, 8:10] = pre.rgb.numpy()[:, 1:3]
    rec[:, 10] = zs if depth_z else 1.0 / zs
    rec[:, 11] = z
    return rec, ranges.numpy(), point_list.numpy(), pre


class Frame:
    """One frame's inputs: records (any float dtype; promoted exactly), ranges [tiles, 2], sorted list, background, size."""

    def __init__(self, rec, ranges, point_list, bg, W, H):
        self.rec = np.asarray(rec)
        self.W, self.H = int(W), int(H)
        self.gx, self.gy = R.tile_grid(W, H)
        self.tiles = self.gx * self.gy
        self.ranges = np.asarray(ranges).astype(np.int64).reshape(self.tiles, 2)
        self.point_list = np.asarray(point_list).astype(np.int64)
        self.bg = np.asarray(bg, dtype=np.float64)

    def tile(self, t):
        """-> (ids [n], pixel x [m], pixel y [m], linear pixel index [m]) of tile t, inside pixels only, row-major"""
        ty, tx = divmod(t, self.gx)
        xs = np.arange(tx * TILE, min(tx * TILE + TILE, self.W))
        ys = np.arange(ty * TILE, min(ty * TILE + TILE, self.H))
        px, py = np.tile(xs, len(ys)), np.repeat(ys, len(xs))
        lo, hi = self.ranges[t]
        return self.point_list[lo:hi], px, py, py * self.W + px


def _consts(dt, published):
    if published:
        return dt(1.0 / 255.0), dt(0.99), dt(1.0e-4)
    return dt(np.float32(1.0) / np.float32(255.0)), dt(np.float32(0.99)), dt(np.float32(0.0001))


def _geometry(rec, ids, px, py, dt, published=False):
    """Everything of a tile's (entry, pixel) pairs that no decision enters, in dtype dt, operation by operation: [n, m] arrays."""
    real = (ids != NO_ID)[:, None]
    r = np.asarray(rec)[np.where(ids != NO_ID, ids, 0)].astype(dt)
    pxf, pyf = px.astype(dt)[None, :], py.astype(dt)[None, :]
    dx, dy = r[:, 0:1] - pxf, r[:, 1:2] - pyf
    A, B, Cc, op = r[:, 2:3], r[:, 3:4], r[:, 4:5], r[:, 5:6]
    amin, acap, _ = _consts(dt, published)
    power = (A * dx + B * dy) * dx + Cc * dy * dy
    with np.errstate(over="ignore", under="ignore"):
        G = np.exp2(np.minimum(power, dt(64.0)))
        alpha = np.minimum(acap, op * G)
    ok = real & (power <= dt(0.0)) & (alpha >= amin)
    return dict(real=real, dx=dx, dy=dy, power=power, G=G, alpha=alpha, ok=ok, col=(r[:, 7], r[:, 8], r[:, 9]), dv=r[:, 10], r=r)


def _doubt(g):
    """(float64 geometry) -> skip-test doubt [n, m], `surely` blended-if-alive [n, m], per-entry relative error bound of 1 - alpha"""
    r, dx, dy = g["r"], g["dx"], g["dy"]
    mag = np.abs(r[:, 2:3]) * dx * dx + np.abs(r[:, 3:4] * dx * dy) + np.abs(r[:, 4:5]) * dy * dy
    amin, acap, _ = _consts(np.float64, False)
    band_p = SAFETY * 8.0 * U * mag
    band_a = SAFETY * (math.log(2.0) * 8.0 * U * mag + 4.0 * U)
    near_p = (mag > 0.0) & (np.abs(g["power"]) <= band_p)
    near_a = np.abs(g["alpha"] / amin - 1.0) <= band_a
    maybe = g["real"] & ((g["power"] <= 0.0) | near_p) & ((g["alpha"] >= amin) | near_a)
    surely = g["ok"] & ~near_p & ~near_a
    capped = g["alpha"] >= acap
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = SAFETY * 2.0 * U + np.where(capped, 0.0, g["alpha"] / (1.0 - g["alpha"]) * band_a)
    return maybe & ~surely, surely, e1


def _forward_columns(g, bg, dt, published=False, ok=None, force_stop=None, e1=None):
    """The forward of the pixels (columns) of `g` under the decisions `ok` (default: the natural ones of dtype dt) and the forced stop
    tests `force_stop` = {(entry, column): bool}.  -> dict of per-column results (+ S scales, + stop-test doubt if e1 is given)"""
    ok = g["ok"] if ok is None else ok
    alpha = g["alpha"]
    n, m = alpha.shape
    one = dt(1.0)
    _, _, thr = _consts(dt, published)
    if n == 0:
        z = np.zeros(m, dtype=dt)
        return dict(color=np.stack([z + dt(bg[c]) for c in range(3)]), depth=z, fT=z + one, nc=np.zeros(m, dtype=np.int64),
                    alpha=z, S_color=np.stack([z + abs(bg[c]) for c in range(3)]), S_depth=z, stop_doubt=[],
                    stopped=np.zeros(m, dtype=bool))
    T_incl = np.cumprod(np.where(ok, one - alpha, one), axis=0, dtype=dt)
    stop = ok & (T_incl < thr)
    if force_stop:
        for (i, j), v in force_stop.items():
            stop[i, j] = v
    stopped = stop.any(axis=0)
    end = np.where(stopped, np.argmax(stop, axis=0), n)              # entries [0, end) can blend
    idx = np.arange(n)[:, None]
    contrib = ok & (idx < end[None, :])
    T_before = np.concatenate([np.ones((1, m), dtype=dt), T_incl[:-1]], axis=0)
    w = np.where(contrib, alpha * T_before, dt(0.0))
    fT = np.where(end > 0, T_incl[np.maximum(end - 1, 0), np.arange(m)], one)
    nc = np.where(contrib, idx + 1, 0).max(axis=0)
    out = dict(fT=fT, nc=nc, alpha=one - fT, stopped=stopped)
    out["color"] = np.stack([np.cumsum(g["col"][c][:, None] * w, axis=0, dtype=dt)[-1] + fT * dt(bg[c]) for c in range(3)])
    out["depth"] = np.cumsum(g["dv"][:, None] * w, axis=0, dtype=dt)[-1]
    out["S_color"] = np.stack([(np.abs(g["col"][c])[:, None] * w).sum(axis=0) + fT * abs(bg[c]) for c in range(3)])
    out["S_depth"] = (np.abs(g["dv"])[:, None] * w).sum(axis=0)
    if e1 is not None:
        # stop tests inside their band, at or before the end of each column, that nothing forces
        Terr = np.cumsum(np.where(ok, e1, 0.0), axis=0)
        near = ok & (np.abs(T_incl / thr - 1.0) <= Terr) & (idx <= np.minimum(end, n - 1)[None, :])
        out["stop_doubt"] = [(int(i), int(j)) for i, j in zip(*np.nonzero(near)) if not (force_stop and (i, j) in force_stop)]
    return out


def _column(g, j):
    return {k: (v[:, j:j + 1] if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[1] > 1 and k != "r" else v)
            for k, v in g.items()}


def forward_reference(frame, published=False):
    """float64 forward of the whole frame.  -> dict: color [3, N], depth, fT, alpha, nc [N] (natural decisions), S_color, S_depth,
    alts = {pixel: [outcome dicts]} for the pixels with doubtful pairs (every assignment, the natural one included), tile_of [N],
    left_out [tiles] bool, doubt [tiles] = number of doubtful pairs"""
    N = frame.W * frame.H
    out = dict(color=np.zeros((3, N)), depth=np.zeros(N), fT=np.ones(N), alpha=np.zeros(N), nc=np.zeros(N, dtype=np.int64),
               S_color=np.zeros((3, N)), S_depth=np.zeros(N), alts={}, tile_of=np.zeros(N, dtype=np.int64),
               left_out=np.zeros(frame.tiles, dtype=bool), doubt=np.zeros(frame.tiles, dtype=np.int64))
    for t in range(frame.tiles):
        ids, px, py, pix = frame.tile(t)
        out["tile_of"][pix] = t
        n_all, m = len(ids), len(pix)
        n = min(n_all, PREFIX)
        while True:
            # (a prefix of the list is the whole answer once every pixel has surely stopped inside it: tile_cull_reference.py)
            g = _geometry(frame.rec, ids[:n], px, py, np.float64, published)
            if n == 0:
                break
            skip_doubt, surely, e1 = _doubt(g)
            # the last entry at which a pixel can still be alive: every doubtful entry skipped, T as large as it can be
            _, _, thr = _consts(np.float64, published)
            T_high = np.cumprod(np.where(surely, 1.0 - g["alpha"], 1.0), axis=0)
            Terr_high = np.cumsum(np.where(surely, e1, 0.0), axis=0)
            late = surely & (T_high * (1.0 + Terr_high) < thr)
            if n == n_all or late.any(axis=0).all():
                break
            n = min(n_all, 4 * n)
        if n == 0:
            f = _forward_columns(g, frame.bg, np.float64, published)
        else:
            f = _forward_columns(g, frame.bg, np.float64, published, e1=e1)
            latest = np.where(late.any(axis=0), np.argmax(late, axis=0), n - 1)
            cand = {}
            for i, j in zip(*np.nonzero(skip_doubt & (np.arange(n)[:, None] <= latest[None, :]))):
                cand.setdefault(int(j), []).append((int(i), "skip"))
            for i, j in f["stop_doubt"]:
                cand.setdefault(j, []).append((i, "stop"))
            d = sum(len(v) for v in cand.values())
            alts = {}
            if d <= MAX_DOUBT:
                for j, pairs in cand.items():
                    res, d_j = _pixel_outcomes(_column(g, j), _column(dict(e1=e1), j)["e1"], frame.bg, pairs, published,
                                               MAX_DOUBT - (d - len(pairs)))
                    d += d_j - len(pairs)
                    if res is None:
                        d = MAX_DOUBT + 1
                        break
                    alts[int(pix[j])] = res
            out["doubt"][t] = d
            if d > MAX_DOUBT:
                out["left_out"][t] = True
            else:
                out["alts"].update(alts)
        for k in ("color", "S_color"):
            out[k][:, pix] = f[k]
        for k in ("depth", "fT", "alpha", "nc", "S_depth"):
            out[k][pix] = f[k]
    return out


def _pixel_outcomes(gc, e1c, bg, pairs, published, room):
    """Every outcome of one pixel (single-column geometry) under the assignments of its doubtful pairs; stop tests that come up
    near their threshold under an assignment join the pairs.  -> (list of outcomes, number of pairs), or (None, .) beyond `room`"""
    pairs = list(pairs)
    while True:
        if len(pairs) > room:
            return None, len(pairs)
        outs, new = [], set()
        for bits in itertools.product((False, True), repeat=len(pairs)):
            ok = gc["ok"].copy()
            fs = {}
            for (i, kind), b in zip(pairs, bits):
                if kind == "skip":
                    ok[i, 0] = b
                else:
                    fs[(i, 0)] = b
            # (a forced stop needs a blended entry: an entry forced to "skip" cannot stop the pixel)
            fs = {k: (v and bool(ok[k[0], 0])) for k, v in fs.items()}
            o = _forward_columns(gc, bg, np.float64, published, ok=ok, force_stop=fs, e1=e1c)
            new |= {(i, "stop") for i, _ in o["stop_doubt"] if (i, "stop") not in pairs}
            outs.append(o)
        if not new:
            return outs, len(pairs)
        pairs += sorted(new)


def forward_replay_f32(frame):
    """The yardstick: the forward in float32 numpy, natural decisions.  -> dict color [3, N], depth, fT, alpha, nc [N]"""
    N = frame.W * frame.H
    out = dict(color=np.zeros((3, N), dtype=np.float32), depth=np.zeros(N, dtype=np.float32), fT=np.ones(N, dtype=np.float32),
               alpha=np.zeros(N, dtype=np.float32), nc=np.zeros(N, dtype=np.int64))
    for t in range(frame.tiles):
        ids, px, py, pix = frame.tile(t)
        n = min(len(ids), PREFIX)
        while True:                                                        # (as above: until every pixel has stopped)
            f = _forward_columns(_geometry(frame.rec, ids[:n], px, py, np.float32), frame.bg.astype(np.float32), np.float32)
            if n == len(ids) or f["stopped"].all():
                break
            n = min(len(ids), 4 * n)
        out["color"][:, pix] = f["color"]
        for k in ("depth", "fT", "alpha", "nc"):
            out[k][pix] = f[k]
    return out


def forward_errors(ref, got):
    """got: color [3, N], depth, fT, alpha, nc [N].  On the tiles not left out: -> ({class: largest |got - ref| / S}, number of pixels
    whose n_contrib matches no assignment).  A doubtful pixel takes the assignment that fits it best."""
    keep = ~ref["left_out"][ref["tile_of"]]

    def figures(r, pix):
        with np.errstate(divide="ignore", invalid="ignore"):
            e = dict(color=np.abs(got["color"][:, pix].astype(np.float64) - r["color"]) / r["S_color"],
                     depth=np.abs(got["depth"][pix].astype(np.float64) - r["depth"]) / r["S_depth"],
                     final_T=np.abs(got["fT"][pix].astype(np.float64) - r["fT"]) / r["fT"],
                     alpha=np.abs(got["alpha"][pix].astype(np.float64) - r["alpha"]) / (1.0 + r["fT"]))
        return {k: np.where(np.isnan(v), 0.0, v) for k, v in e.items()}          # (0 / 0: nothing blended, nothing written)
    pix = np.arange(len(keep))
    e = figures(ref, pix)
    bad_nc = (np.asarray(got["nc"]).astype(np.int64) != ref["nc"])
    for p, outs in ref["alts"].items():
        best = None
        for o in outs:
            if int(o["nc"][0]) != int(got["nc"][p]):
                continue
            eo = figures({k: (v[:, 0] if v.ndim == 2 and k in ("color", "S_color") else v[0]) for k, v in o.items()
                          if k not in ("stop_doubt", "stopped")}, p)
            worst = max(float(np.max(v)) for v in eo.values())
            if best is None or worst < best[0]:
                best = (worst, eo)
        bad_nc[p] = best is None
        if best is not None:
            for k in e:
                e[k][..., p] = best[1][k]
    fig = {k: float(np.max(np.where(keep, v, 0.0))) if keep.any() else 0.0 for k, v in e.items()}
    return fig, int((bad_nc & keep).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _backward_columns(g, ok, nc, fT, gp, gd, gA, bg, dt, scales):
    """Per-pixel terms of the gradient records of the columns of `g`: entries [0, n) back to front, blended where ok and entry <= nc.
    gp [3, m], gd, gA [m] (zeros: absent).  -> V [10, n, m] (dt) and, if scales, the magnitudes Sabs [10, n, m] (float64)"""
    n, m = g["alpha"].shape
    zero, one = dt(0.0), dt(1.0)
    act = ok & (np.arange(1, n + 1)[:, None] <= nc[None, :])
    a = np.where(act, g["alpha"], zero)
    Ge = np.where(act, g["G"], zero)
    rcp = one / (one - a)
    # T after entry i's division = final_T times the reciprocals of entries n - 1 .. i, one product at a time
    T = (np.cumprod(np.concatenate([fT[None, :].astype(dt), rcp[::-1]], axis=0), axis=0, dtype=dt)[1:])[::-1]
    dch = a * T
    c0, c1, c2 = (c[:, None] for c in g["col"])
    cg = c0 * gp[0][None, :] + c1 * gp[1][None, :] + c2 * gp[2][None, :] + g["dv"][:, None] * gd[None, :]
    nTb = -fT.astype(dt) * ((dt(bg[0]) * gp[0] + dt(bg[1]) * gp[1] + dt(bg[2]) * gp[2]) - gA)
    diff = np.empty((n, m), dtype=dt)
    S = np.zeros(m, dtype=dt)
    for i in range(n - 1, -1, -1):
        diff[i] = cg[i] - S
        S = S + a[i] * diff[i]
    h = Ge * (diff * T + nTb[None, :] * rcp)
    dx, dy = g["dx"], g["dy"]
    v0, v1 = h * dx, h * dy
    V = np.stack([v0, v1, v0 * dx, v0 * dy, v1 * dy, h, dch * gp[0][None, :], dch * gp[1][None, :], dch * gp[2][None, :],
                  dch * gd[None, :]])
    if not scales:
        return V, None
    cga = (np.abs(c0 * gp[0][None, :]) + np.abs(c1 * gp[1][None, :]) + np.abs(c2 * gp[2][None, :])
           + np.abs(g["dv"][:, None] * gd[None, :]))
    nTa = fT * (abs(bg[0]) * np.abs(gp[0]) + abs(bg[1]) * np.abs(gp[1]) + abs(bg[2]) * np.abs(gp[2]) + np.abs(gA))
    Sa_before = np.empty((n, m))
    Sa = np.zeros(m)
    for i in range(n - 1, -1, -1):
        Sa_before[i] = Sa
        Sa = Sa + a[i] * (cga[i] - Sa)
    ha = Ge * ((cga + Sa_before) * T + nTa[None, :] * rcp)
    adx, ady = np.abs(dx), np.abs(dy)
    Sabs = np.stack([ha * adx, ha * ady, ha * dx * dx, ha * adx * ady, ha * dy * dy, ha, dch * np.abs(gp[0])[None, :],
                     dch * np.abs(gp[1])[None, :], dch * np.abs(gp[2])[None, :], dch * np.abs(gd)[None, :]])
    return V, Sabs


def _tile_state(frame, t, nc, fT, grads):
    ids, px, py, pix = frame.tile(t)
    gp, gd, gA = grads
    zeros = np.zeros(len(pix), dtype=np.float32)
    return (ids, px, py, pix, np.asarray(nc).reshape(-1)[pix].astype(np.int64), np.asarray(fT).reshape(-1)[pix],
            gp.reshape(3, -1)[:, pix], zeros if gd is None else gd.reshape(-1)[pix], zeros if gA is None else gA.reshape(-1)[pix])


def backward_reference(frame, nc, fT, grads, published=False):
    """float64 records of every tile from the frame's n_contrib / final_T [H, W] and grads = (dL/dcolour [3, H, W], dL/d(depth plane)
    [H, W] or None, dL/d(alpha plane) [H, W] or None).  -> list over tiles of dict: walk (entries with a record = the deepest n_contrib
    of the tile, at most the list), base [walk, 20] (values and magnitudes summed over the pixels without doubt), alts = list over
    the doubtful pixels of [2^k arrays [walk, 20]] (natural = the index of float64's own decisions among them), doubt, left_out"""
    out = []
    for t in range(frame.tiles):
        ids, px, py, pix, nct, fTt, gp, gd, gA = _tile_state(frame, t, nc, fT, grads)
        walk = int(min(len(ids), nct.max())) if len(ids) else 0
        if walk == 0:
            out.append(dict(walk=0, base=np.zeros((0, 20)), alts=[], doubt=0, left_out=False))
            continue
        g = _geometry(frame.rec, ids[:walk], px, py, np.float64, published)
        f64 = [x.astype(np.float64) for x in (fTt, gp, gd, gA)]
        skip_doubt, _, _ = _doubt(g)
        skip_doubt &= np.arange(1, walk + 1)[:, None] <= nct[None, :]
        V, Sabs = _backward_columns(g, g["ok"], nct, f64[0], f64[1], f64[2], f64[3], frame.bg, np.float64, True)
        VS = np.concatenate([V, Sabs])                                     # [20, walk, m]
        d = int(skip_doubt.sum())
        cols = sorted(set(int(j) for j in np.nonzero(skip_doubt)[1]))
        res = dict(walk=walk, doubt=d, left_out=d > MAX_DOUBT, alts=[], natural=[])
        if d > MAX_DOUBT:
            cols = []
        plain = np.ones(len(pix), dtype=bool)
        plain[cols] = False
        res["base"] = VS[:, :, plain].sum(axis=2).T
        for j in cols:
            entries = [int(i) for i in np.nonzero(skip_doubt[:, j])[0]]
            gc = _column(g, j)
            variants = []
            for bits in itertools.product((False, True), repeat=len(entries)):
                ok = gc["ok"].copy()
                ok[entries, 0] = bits
                v, s = _backward_columns(gc, ok, nct[j:j + 1], f64[0][j:j + 1], f64[1][:, j:j + 1], f64[2][j:j + 1],
                                         f64[3][j:j + 1], frame.bg, np.float64, True)
                variants.append(np.concatenate([v, s])[:, :, 0].T)
            res["alts"].append(variants)
            res["natural"].append(int(sum(int(b) << (len(entries) - 1 - k) for k, b in enumerate(g["ok"][entries, j]))))
        out.append(res)
    return out


def natural_records(ref):
    """backward_reference's result -> list over tiles of records [walk, 10] under float64's own decisions"""
    return [r["base"][:, :10] + sum((v[i][:, :10] for v, i in zip(r["alts"], r["natural"])), np.zeros((r["walk"], 10))) for r in ref]


def backward_replay_f32(frame, nc, fT, grads):
    """The yardstick: float32 numpy, natural decisions, the pixels of a tile added one after the other in row-major order.
    -> list over tiles of records [walk, 10] float32"""
    out = []
    for t in range(frame.tiles):
        ids, px, py, pix, nct, fTt, gp, gd, gA = _tile_state(frame, t, nc, fT, grads)
        walk = int(min(len(ids), nct.max())) if len(ids) else 0
        if walk == 0:
            out.append(np.zeros((0, 10), dtype=np.float32))
            continue
        g = _geometry(frame.rec, ids[:walk], px, py, np.float32)
        V, _ = _backward_columns(g, g["ok"], nct, fTt.astype(np.float32), gp.astype(np.float32), gd.astype(np.float32),
                                 gA.astype(np.float32), frame.bg.astype(np.float32), np.float32, False)
        out.append(np.cumsum(V, axis=2, dtype=np.float32)[:, :, -1].T)
    return out


def backward_errors(ref, got):
    """got: list over tiles of records [>= walk, 10] (list order).  -> ({value name: largest |got - ref| / S over the tiles not left
    out}, the records of the chosen assignment per tile (None: left out))"""
    fig = {k: 0.0 for k in RECORD_VALUES}
    chosen = []
    for r, gt in zip(ref, got):
        if r["left_out"] or r["walk"] == 0:
            chosen.append(None if r["left_out"] else np.zeros((0, 10)))
            continue
        gt = np.asarray(gt[:r["walk"]], dtype=np.float64)
        best = None
        for pick in itertools.product(*[range(len(v)) for v in r["alts"]]):
            tot = r["base"] + sum((r["alts"][k][p] for k, p in enumerate(pick)), np.zeros_like(r["base"]))
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.abs(gt - tot[:, :10]) / tot[:, 10:]
            e = np.where(np.isnan(e), 0.0, e).max(axis=0)
            if best is None or e.max() < best[0].max():
                best = (e, tot[:, :10])
        for k, v in zip(RECORD_VALUES, best[0]):
            fig[k] = max(fig[k], float(v))
        chosen.append(best[1])
    return fig, chosen


def instances(frame):
    """-> (tile [R], position in the tile's list [R], Gaussian id [R]) of every list position, list order"""
    lens = frame.ranges[:, 1] - frame.ranges[:, 0]
    tile = np.repeat(np.arange(frame.tiles), lens)
    pos = np.arange(len(tile)) - np.repeat(frame.ranges[:, 0] - frame.ranges[0, 0], lens)
    return tile, pos, frame.point_list[frame.ranges[0, 0]:frame.ranges[0, 0] + len(tile)]


def mean2d_from_records(frame, records, slot, dt):
    """records [R, 10] in list order (zeros behind a tile's walk), slot [R] = the emission slot of every list position (ascending
    inside a Gaussian).  The per-Gaussian sums in slot order and the moment-to-mean map, in dtype dt.
    -> (dL/dmean2D [P, 2] dt, scale [P, 2] float64 = the sum of the magnitudes of the map's terms, sums [P, 10] dt)"""
    _, _, gid = instances(frame)
    real = gid != NO_ID
    order = np.argsort(np.asarray(slot)[real], kind="stable")
    gid, recs = gid[real][order], np.asarray(records)[real][order]
    P = frame.rec.shape[0]
    acc = np.zeros((P, 10), dtype=dt)
    np.add.at(acc, gid, recs.astype(dt))                                   # (unbuffered: one addition per record, in slot order)
    mag = np.zeros((P, 2))
    np.add.at(mag, gid, np.abs(recs[:, 0:2].astype(np.float64)))
    r = frame.rec.astype(dt)
    cA, cB, cC = dt(-2.0) * r[:, 2] / dt(LOG2E), -r[:, 3] / dt(LOG2E), dt(-2.0) * r[:, 4] / dt(LOG2E)
    m0, m1 = acc[:, 0] * r[:, 5], acc[:, 1] * r[:, 5]
    gm = np.stack([dt(0.5 * frame.W) * (-cA * m0 - cB * m1), dt(0.5 * frame.H) * (-cC * m1 - cB * m0)], axis=1)
    r64 = frame.rec.astype(np.float64)
    a64 = np.abs(np.stack([-2.0 * r64[:, 2], -r64[:, 3], -2.0 * r64[:, 4]], axis=1) / LOG2E) * np.abs(r64[:, 5:6])
    scale = np.stack([0.5 * frame.W * (a64[:, 0] * mag[:, 0] + a64[:, 1] * mag[:, 1]),
                      0.5 * frame.H * (a64[:, 2] * mag[:, 1] + a64[:, 1] * mag[:, 0])], axis=1)
    return gm, scale, acc


def mean2d_error(frame, records, slot, got):
    """|got - float64 map of the float64 slot-order sums of `records`| / scale, largest over the Gaussians with a non-zero scale"""
    ref, scale, _ = mean2d_from_records(frame, records, slot, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(np.asarray(got, dtype=np.float64)[:, :2] - ref) / scale
    return float(np.max(np.where(scale > 0.0, e, 0.0), initial=0.0))


def oracle_slots(frame):
    """Emission slots as the oracle emits: ascending Gaussian id, row-major over the tiles of its rectangle"""
    tile, _, gid = instances(frame)
    order = np.lexsort((tile, gid))
    slot = np.empty(len(gid), dtype=np.int64)
    slot[order] = np.arange(len(gid))
    return slot


def records_in_list_order(frame, per_tile):
    """list over tiles of [walk, 10] -> [R, 10] in list order, zeros behind every walk"""
    out = np.zeros((int((frame.ranges[:, 1] - frame.ranges[:, 0]).sum()), 10), dtype=np.float64)
    base = frame.ranges[0, 0]
    for t, r in enumerate(per_tile):
        if r is not None and len(r):
            lo = frame.ranges[t, 0] - base
            out[lo:lo + len(r)] = r
    return out


def yardstick(name, verbose=False):
    """One case on the CPU: the oracle's records rounded to float32 (what a frame holds), the float64 replay against the float32
    replay - forward, backward without and with the depth-plane / alpha-plane gradients, the per-Gaussian sums and the map.
    -> ({class: largest figure of the float32 replay}, {stage: tiles left out}, tiles)"""
    raw, cam, deg, W, H, bg = case_scene(name)
    rec, ranges, point_list, _ = oracle_frame(raw, cam, deg, W, H)
    frame = Frame(rec.astype(np.float32), ranges, point_list, bg, W, H)
    ref, f32 = forward_reference(frame), forward_replay_f32(frame)
    fig, bad = forward_errors(ref, f32)
    assert bad == 0, (name, bad)
    left = dict(forward=int(ref["left_out"].sum()))
    gp, gd, gA = upstream(W, H)
    slot = oracle_slots(frame)
    for extras in (False, True):
        grads = (gp, gd if extras else None, gA if extras else None)
        bref = backward_reference(frame, f32["nc"], f32["fT"], grads)
        b32 = backward_replay_f32(frame, f32["nc"], f32["fT"], grads)
        bfig, _ = backward_errors(bref, b32)
        recs = records_in_list_order(frame, b32)
        gm, _, _ = mean2d_from_records(frame, recs, slot, np.float32)
        bfig["mean2D"] = mean2d_error(frame, recs, slot, gm)
        for k, v in bfig.items():
            fig[k] = max(fig.get(k, 0.0), v)
        left["backward+extras" if extras else "backward"] = sum(r["left_out"] for r in bref)
    if verbose:
        print(f"{name}: tiles {frame.tiles}, left out {left}, " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    return fig, left, frame.tiles


def bounds(yardstick):
    """{class: float32 replay's largest figure} -> {class: bound}"""
    return {k: max(FLOOR, FACTOR * v) for k, v in yardstick.items()}
