"""The inputs and the case table of tests/test_frame_paths_pinned_gpu.py: one small scene sent through every exported forward and
backward entry point of the rasterizer (include/gsr.h) and every host-side route behind them (csrc/api.hip).  numpy only.

Scene: 200 Gaussians from a fixed seed, anisotropic scales, 80 of them a nearly opaque wall in front of the camera, of the others
about a sixth behind the camera and a good part off-screen, SH degree 1
in the raw-parameter call form (`dc` + `shs` separately, raw opacity / scaling / rotation: what the folded Adam step needs), image
24 x 20 = 2 x 2 tiles with both edges partial.  What is pinned are host-routing mistakes - a wrong pointer, flag or stage order -
and those show at any size."""
import functools
import itertools

import numpy as np

P, W, H, SH_DEGREE, SH_REST = 200, 24, 20, 1, 3
WALL = 80
TANFOV = 0.5
TILES = ((W + 15) // 16) * ((H + 15) // 16)
CAPACITY = 4096                      # well above the frame's instance count (test_the_scene_is_what_the_cases_need checks it)
SMALL_CAPACITY = 64                  # below it: the frame that is rendered again
TOUCHED_T_MIN = 0.25
ADAM_LR = (1.6e-4, 2.5e-3, 1.25e-4, 2.5e-2, 5e-3, 1e-3)
ADAM_STEP = (3, 3, 3, 3, 3, 3)
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-15


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict of float32 arrays: the Gaussians, the upstream gradients, the Adam moments.  Shared: do not write."""
    rng = np.random.default_rng(20261020)
    z = rng.uniform(-1.0, 5.0, size=P)
    xy = rng.uniform(-1.0, 1.0, size=(P, 2)) * np.abs(z)[:, None] * 0.9       # |x / z| up to 0.9: tan(fov / 2) is 0.5
    means = np.concatenate([xy, z[:, None]], axis=1)
    scales = np.log(rng.uniform(0.02, 0.12, size=(P, 3)) * np.array([1.0, 3.0, 0.3]))
    opacities = 2.0 * rng.standard_normal((P, 1))
    # the first WALL of them: large, nearly opaque, in front of the camera - every tile's list gets long enough and its pixels
    # saturate early enough for the depth cut-off of gsr_forward_async_culled to bite
    z[:WALL] = rng.uniform(0.5, 4.0, size=WALL)
    means[:WALL] = np.concatenate([rng.uniform(-0.3, 0.3, size=(WALL, 2)) * z[:WALL, None], z[:WALL, None]], axis=1)
    scales[:WALL] = np.log(rng.uniform(0.3, 0.6, size=(WALL, 3)) * np.array([1.0, 2.0, 0.5]))
    opacities[:WALL] = 5.0
    out = dict(means3D=means, scales=scales, rotations=rng.standard_normal((P, 4)), opacities=opacities,
               dc=0.8 * rng.standard_normal((P, 1, 3)), shs=0.3 * rng.standard_normal((P, SH_REST, 3)),
               bg=np.array([0.1, 0.2, 0.3]), dL_dcolor=rng.standard_normal((3, H, W)), dL_ddepth=rng.standard_normal((1, H, W)),
               dL_dalpha=rng.standard_normal((H, W)))
    for k, shape in (("xyz", (P, 3)), ("f_dc", (P, 1, 3)), ("f_rest", (P, SH_REST, 3)), ("opacity", (P, 1)), ("scaling", (P, 3)),
                     ("rotation", (P, 4))):
        out["m_" + k] = 1e-3 * rng.standard_normal(shape)
        out["v_" + k] = 1e-6 * rng.random(shape)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


ADAM_GROUPS = (("xyz", "means3D"), ("f_dc", "dc"), ("f_rest", "shs"), ("opacity", "opacities"), ("scaling", "scales"),
               ("rotation", "rotations"))      # gsr_fused_adam's group order -> the array of scene() that is the parameter


@functools.lru_cache(maxsize=None)
def camera(kind="front"):
    """-> dict(viewmatrix, projmatrix [16] row-major transposed as the settings take them, campos [3]) float32.
    front: at the origin, looking down +z.  away: 50 units in front of the scene, so every Gaussian lies behind it."""
    w2c = np.eye(4)
    if kind == "away":
        w2c[2, 3] = -50.0
    znear, zfar = 0.01, 100.0
    proj = np.zeros((4, 4))
    proj[0, 0] = proj[1, 1] = 1.0 / TANFOV
    proj[3, 2] = 1.0
    proj[2, 2] = zfar / (zfar - znear)
    proj[2, 3] = -(zfar * znear) / (zfar - znear)
    campos = np.linalg.inv(w2c)[:3, 3]
    return {k: np.ascontiguousarray(v, dtype=np.float32).ravel()
            for k, v in dict(viewmatrix=w2c.T, projmatrix=(proj @ w2c).T, campos=campos).items()}


# ---- forward cases ------------------------------------------------------------------------------------------------------------------
# variant: "plain" = the entry points without _ex; "ex" = the _ex twins with GSR_DEPTH_Z, out_alpha and n_touched; "exnull" = the _ex
# twins with extras = NULL
VARIANTS = ("plain", "ex", "exnull")
STATUS_KINDS = ("null", "pinned", "pageable")


def _forward_cases():
    c = {}
    for v in VARIANTS:
        c[f"prepare_render_fb0_{v}"] = dict(path="blocking", shade="fused", fb=0, variant=v)
        c[f"prepare_render_fb1_{v}"] = dict(path="blocking", shade="fused", fb=1, variant=v)
        c[f"geometry_shade_render_{v}"] = dict(path="blocking", shade="call", fb=1, variant=v)
        c[f"geometry_render_shade_noevent_{v}"] = dict(path="blocking", shade="late", event=False, fb=1, variant=v)
        c[f"geometry_render_shade_event_{v}"] = dict(path="blocking", shade="late", event=True, fb=1, variant=v)
        for tlo, count, status, defer, aside in itertools.product((0, 1), (0, 1), STATUS_KINDS, (0, 1), (0, 1)):
            c[f"async_tlo{tlo}_count{count}_{status}_defer{defer}_aside{aside}_{v}"] = dict(
                path="async", tlo=tlo, count=count, status=status, defer=defer, aside=aside, fb=1, variant=v)
        for tlo in (0, 1):
            c[f"overflow_rerender_tlo{tlo}_{v}"] = dict(path="rerender", tlo=tlo, fb=1, variant=v)
        c[f"culled_{v}"] = dict(path="culled", fb=1, variant=v)
        c[f"sees_nothing_blocking_{v}"] = dict(path="blocking", shade="fused", fb=1, variant=v, camera="away")
        c[f"sees_nothing_async_{v}"] = dict(path="async", tlo=1, count=1, status="pinned", defer=0, aside=0, fb=1, variant=v,
                                            camera="away")
        c[f"no_gaussians_blocking_{v}"] = dict(path="blocking", shade="fused", fb=1, variant=v, P=0)
        c[f"no_gaussians_async_{v}"] = dict(path="async", tlo=1, count=1, status="pinned", defer=0, aside=0, fb=1, variant=v, P=0)
    c["debug_blocking_ex"] = dict(path="blocking", shade="fused", fb=1, variant="ex", debug=1)
    c["debug_async_tlo0_ex"] = dict(path="async", tlo=0, count=1, status="pinned", defer=0, aside=0, fb=1, variant="ex", debug=1)
    c["debug_async_tlo1_plain"] = dict(path="async", tlo=1, count=0, status="pageable", defer=0, aside=0, fb=1, variant="plain",
                                       debug=1)
    return c


FORWARD_CASES = _forward_cases()

# ---- backward cases: every form on five frames made for a backward, each in the three variants -----------------------------------------
BACKWARD_FRAMES = {"blocking": "prepare_render_fb1", "async_tlo0": "async_tlo0_count1_pinned_defer0_aside0",
                   "async_tlo1": "async_tlo1_count0_pinned_defer0_aside0", "rerender_tlo1": "overflow_rerender_tlo1",
                   "culled": "culled"}
BACKWARD_FORMS = ("plain", "camera", "camera_only", "adam_sparse0", "adam_sparse1", "adam_sparse2_culled_rows")
BACKWARD_CASES = {f"backward_{form}_on_{frame}_{v}": dict(frame=f"{fwd}_{v}", form=form, variant=v)
                  for (frame, fwd), form, v in itertools.product(BACKWARD_FRAMES.items(), BACKWARD_FORMS, VARIANTS)}
BACKWARD_CASES["backward_plain_on_no_gaussians_plain"] = dict(frame="no_gaussians_blocking_plain", form="plain", variant="plain")
BACKWARD_CASES["backward_camera_on_no_gaussians_ex"] = dict(frame="no_gaussians_blocking_ex", form="camera", variant="ex")
BACKWARD_CASES["backward_camera_on_sees_nothing_plain"] = dict(frame="sees_nothing_blocking_plain", form="camera", variant="plain")

DYNAMIC_CASES = {"adam_set_dynamic_sparse0": 0, "adam_set_dynamic_sparse1": 1}

NAMES = tuple(FORWARD_CASES) + tuple(BACKWARD_CASES) + tuple(DYNAMIC_CASES)


# ---- what the fixture remembers of the inputs ---------------------------------------------------------------------------------------
def checksum(a):
    return float(np.asarray(a, dtype=np.float64).sum())


def input_checksums():
    """{key: float64} over every input array"""
    out = {f"sum_scene_{k}": checksum(v) for k, v in scene().items()}
    for kind in ("front", "away"):
        out.update({f"sum_camera_{kind}_{k}": checksum(v) for k, v in camera(kind).items()})
    out["sum_adam"] = checksum(ADAM_LR + ADAM_STEP + (ADAM_BETA1, ADAM_BETA2, ADAM_EPS))
    return out
