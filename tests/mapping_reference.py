"""CPU restatements for the mapping tests (float64 numpy / torch): brute-force 3-nearest-neighbour mean squared distance, and
the back-projection + selection rule of an RGB-D keyframe.  Independent of the library: nothing here calls the HIP path."""
import math

import numpy as np
import torch


def knn_dist2_bruteforce(points, first_query=0, chunk=None, device="cpu"):
    """points [P,3] (any float type; evaluated in float64 on exactly these values) -> float64 [P - first_query] on the CPU: mean
    of the min(3, P-1) smallest squared distances from row i to the rows with another index; 0 for P == 1.  Distances from
    differences, never |a|^2 + |b|^2 - 2ab.  `device`: where torch evaluates the float64 arithmetic (a large set takes minutes on
    the CPU); the algorithm is the same quadratic one."""
    x = points.detach() if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
    x = x.to(device=device, dtype=torch.float64)
    P = x.shape[0]
    k = min(3, P - 1)
    out = torch.zeros(P - first_query, dtype=torch.float64, device=device)
    if k == 0:
        return out.cpu()
    chunk = chunk or max(1, min(4096, (1 << 25) // P))
    for s in range(first_query, P, chunk):
        q = x[s:s + chunk]
        d = torch.zeros((q.shape[0], P), dtype=torch.float64, device=device)
        for a in range(3):
            d += (q[:, a:a + 1] - x[None, :, a]) ** 2
        rows = torch.arange(q.shape[0], device=device)
        d[rows, rows + s] = math.inf                                           # the row itself (a duplicate elsewhere counts)
        out[s - first_query:s - first_query + q.shape[0]] = torch.topk(d, k, dim=1, largest=False).values.sum(1) / k
    return out.cpu()


def last_sorted_row(points):
    """points float32 [P,3], all finite -> the row that the neighbour structure of csrc/knn.hip sorts LAST: the largest 30-bit
    Morton code of the cells (v - lo) / (hi - lo) * 1023 (float32, one rounding per operation) in the cloud's bounding box, on
    equal codes the largest row (the sort is stable).  With P = 64 * 64 * n + 1 it is the one point of the last super-box."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    lo, hi = p.min(axis=0), p.max(axis=0)
    t = (p - lo) / (hi - lo) * np.float32(1023.0)
    cell = np.where(t >= 0, np.minimum(t, np.float32(1023.0)), np.float32(0)).astype(np.uint32)

    def spread(x):
        x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
        x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
        x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
        return (x | (x << np.uint32(2))) & np.uint32(0x09249249)

    code = spread(cell[:, 0]) | (spread(cell[:, 1]) << np.uint32(1)) | (spread(cell[:, 2]) << np.uint32(2))
    return int(np.flatnonzero(code == code.max())[-1])


def selection_mask(depth, alpha=None, rendered_z=None, stride=1, min_depth=0.2, max_depth=math.inf, alpha_below=0.5,
                   front_margin=0.05, dtype=np.float64):
    """[H,W] bool: the strided pixels gsr_unproject_rgbd selects, evaluated in `dtype`."""
    d = np.asarray(depth, dtype=dtype).reshape(depth.shape[-2:])
    H, W = d.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        valid = np.isfinite(d) & (d > dtype(min_depth)) & (d <= dtype(max_depth))
        if alpha is None:
            sel = valid
        else:
            A = np.asarray(alpha, dtype=dtype).reshape(H, W)
            sel = A < dtype(alpha_below)
            if rendered_z is not None:
                z = np.asarray(rendered_z, dtype=dtype).reshape(H, W)
                sel = sel | (d < z / A - dtype(front_margin) * d)
            sel = valid & sel
    grid = np.zeros((H, W), dtype=bool)
    grid[::stride, ::stride] = True
    return sel & grid


def unproject_reference(cam, image, depth, **selection):
    """-> (xyz float64 [n,3], rgb [n,3] in the image's dtype, mask [H,W]) in row-major pixel order.  Pixel centres at integer
    coordinates: ndc = (2 p + 1) / S - 1; p_view = (ndc_x tanfovx d, ndc_y tanfovy d, d); p_world = R^T (p_view - t)."""
    img = np.asarray(image)
    d = np.asarray(depth, dtype=np.float64).reshape(depth.shape[-2:])
    H, W = d.shape
    mask = selection_mask(np.asarray(depth), **selection)
    ys, xs = np.nonzero(mask)                                               # row-major
    dd = d[ys, xs]
    ndc_x, ndc_y = (2.0 * xs + 1.0) / W - 1.0, (2.0 * ys + 1.0) / H - 1.0
    pv = np.stack([ndc_x * math.tan(cam.FoVx * 0.5) * dd, ndc_y * math.tan(cam.FoVy * 0.5) * dd, dd], axis=1)
    V = np.asarray(cam.world_view_transform.detach().cpu(), dtype=np.float64)      # W2C^T: p_view = p_world V[:3,:3] + V[3,:3]
    xyz = (pv - V[3, :3]) @ V[:3, :3].T
    return xyz, img[:, ys, xs].T.copy(), mask


def project_to_pixels(cam, xyz):
    """World points -> (pixel x, pixel y, view z) float64 through the project's projection convention (scene_utils.cameras:
    full_proj_transform, ndc -> pixel ((ndc + 1) S - 1) / 2)."""
    x = np.asarray(xyz, dtype=np.float64)
    F = np.asarray(cam.full_proj_transform.detach().cpu(), dtype=np.float64)
    V = np.asarray(cam.world_view_transform.detach().cpu(), dtype=np.float64)
    h = x @ F[:3] + F[3]
    ndc = h[:, :2] / h[:, 3:4]
    W, H = cam.image_width, cam.image_height
    return ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5, x @ V[:3, 2] + V[3, 2]


def depth_sheet(H, W, seed=0, invalid_frac=0.0, base=2.0, amp=0.6):
    """A smooth synthetic depth image [H,W] float32 (a 2-D sheet once back-projected), optionally with invalid readings (0, NaN,
    a far outlier) scattered in."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = base + amp * np.sin(x / W * 5.0 + rng.uniform(0, 6)) * np.cos(y / H * 4.0 + rng.uniform(0, 6)) + \
        0.02 * rng.standard_normal((H, W))
    d = d.astype(np.float32)
    if invalid_frac > 0:
        r = rng.uniform(size=(H, W))
        d[r < invalid_frac] = 0.0
        d[(r >= invalid_frac) & (r < 2 * invalid_frac)] = np.nan
        d[(r >= 2 * invalid_frac) & (r < 3 * invalid_frac)] = 1.0e4
    return d
