"""The native surface of `simple_knn`: `distCUDA2(points)` as the reference calls it, and `knn_dist2(points, first_query)`,
the same search answered only for the rows from `first_query` on (new points against map + new points)."""
import torch

from diff_gaussian_rasterization import _C as _gsr


def knn_dist2(points, first_query=0):
    """points [P,3] float on the HIP device -> float32 [P - first_query]: for every row i >= first_query the mean of the three
    smallest squared distances to the OTHER rows of `points` (exact neighbours; min(3, P-1) of them when P < 4, 0 for P == 1).
    Equal to `knn_dist2(points)[first_query:]` bit for bit."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _gsr.GsrError("simple_knn needs a tensor on the HIP device (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [P, 3], got {tuple(points.shape)}")
    pts = points.detach().float().contiguous()
    P, first = int(pts.shape[0]), int(first_query)
    if P == 0 and first == 0:
        return torch.empty(0, dtype=torch.float32, device=pts.device)
    if not 0 <= first < P:
        raise ValueError(f"first_query={first_query}: expected a row of the {P} points")
    lib = _gsr.lib()
    out = torch.empty(P - first, dtype=torch.float32, device=pts.device)
    with _gsr.on_device(pts.device):
        ws = torch.empty(lib.gsr_knn_workspace_bytes(P), dtype=torch.uint8, device=pts.device)
        _gsr.check(lib.gsr_knn_dist2(P, _gsr.ptr(pts), first, _gsr.ptr(out), _gsr.ptr(ws), ws.numel(), _gsr._stream()))
    return out


def distCUDA2(points):
    """reference scene/gaussian_model.py:140: mean squared distance of every point to its three nearest neighbours."""
    return knn_dist2(points, 0)
