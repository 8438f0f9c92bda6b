"""How the point-cloud and tracking front ends reject an argument: the one place that words a TypeError for a value that is no
number, a ValueError for one out of range or a tensor of the wrong shape, and a GsrError for a tensor that is not on the HIP
device.  Nothing here loads the native library or allocates on a device before the argument has passed; `device_T` alone
allocates, and is called after everything else has."""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch


def gsr():
    from diff_gaussian_rasterization import _C
    return _C


def is_number(value):
    return isinstance(value, numbers.Real) and not isinstance(value, bool)


def is_integer(value):
    return isinstance(value, numbers.Integral) and not isinstance(value, bool)


def number(name, value, ok=None, expected=None):
    """-> float(value).  TypeError unless it is a real number (a bool is none); ValueError, printing the value as given, unless
    ok(value) - the range rule, which stays at the call site (None: any number, NaN included)."""
    if not is_number(value):
        raise TypeError(f"{name}={value!r}: expected a number")
    if ok is not None and not ok(value):
        raise ValueError(f"{name}={value}: expected {expected}")
    return float(value)


def integer(name, value, lo, hi=None, expected=None):
    """-> int(value).  TypeError unless it is an integer (a bool is none); ValueError outside lo .. hi (hi=None: no upper bound)."""
    if not is_integer(value):
        raise TypeError(f"{name}={value!r}: expected an int")
    if value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name}={value}: expected " + (expected or (f">= {lo}" if hi is None else f"{lo} .. {hi}")))
    return int(value)


def voxel_size(value):
    return number("voxel_size", value, lambda v: math.isfinite(v) and v > 0, "a finite value > 0")


def neighbourhood(radius, max_nn, lo, hi, names=("radius", "max_nn"), radius_alone=False):
    """The hybrid neighbourhood of estimate_normals and its users -> (radius, max_nn): the rows within radius (> 0, inf allowed),
    cut at the max_nn (lo .. hi) nearest.  radius_alone: max_nn = 0 switches the cut off, and the radius must then be finite."""
    r = number(names[0], radius, lambda v: v > 0,      # (false for NaN)
               "a value > 0" + ("" if radius_alone else f" (inf: limited by {names[1]} only)"))
    if radius_alone and is_integer(max_nn) and max_nn == 0:
        if math.isinf(r):
            raise ValueError(f"{names[1]}=0 (the radius alone) needs a finite radius")
        return r, 0
    return r, integer(names[1], max_nn, lo, hi, f"{lo} .. {hi}, or 0 for the radius alone" if radius_alone else None)


def rows(cloud):
    return int(cloud.shape[0]) if isinstance(cloud, torch.Tensor) and cloud.dim() == 2 else None


def tensor(t, name, shape, note="", also=None, convert=True):
    """A floating-point tensor of `shape` (or of the shape `also`) on the HIP device -> contiguous float32.  An entry of `shape`
    that is a string stands for any size and is printed as it is: ("P", 3).  Type and shape first (ValueError, ending in `note`),
    then the device (GsrError); convert=False is that first pass alone, for callers that look at every shape before any device."""
    if not isinstance(t, torch.Tensor) or not t.is_floating_point() or not any(
            s is not None and t.dim() == len(s) and all(isinstance(n, str) or int(d) == n for d, n in zip(t.shape, s))
            for s in (shape, also)):
        raise ValueError(f"{name}: expected a floating-point tensor of shape ({', '.join(str(n) for n in shape)}){note}")
    if not convert:
        return None
    if not t.is_cuda:
        raise gsr().GsrError(f"{name} must live on the HIP device (no CPU path)")
    return t.detach().float().contiguous()


def cloud(points, colors, who):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise gsr().GsrError(f"{who} needs points on the HIP device (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [P, 3], got {tuple(points.shape)}")
    pts = points.detach().float().contiguous()
    col = None
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or not colors.is_cuda:
            raise gsr().GsrError(f"{who} needs colors on the HIP device (no CPU path)")
        if tuple(colors.shape) != tuple(points.shape):
            raise ValueError(f"colors: expected {tuple(points.shape)} like points, got {tuple(colors.shape)}")
        col = colors.detach().float().to(pts.device).contiguous()
    return pts, col


def nonempty(pts, who, what):
    if int(pts.shape[0]) == 0:
        raise ValueError(f"{who}: the {what} cloud is empty")


def transform(T, name="transformation"):
    """None, or anything that gives a [4,4] matrix -> None / (tensor or array as given); shape and type only"""
    if T is None:
        return None
    if not isinstance(T, torch.Tensor):
        T = torch.as_tensor(T, dtype=torch.float64)
    if tuple(T.shape) != (4, 4) or not T.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point [4,4] matrix, got {T.dtype} {tuple(T.shape)}")
    return T


def device_T(T, dev):
    """a fresh contiguous float64 [4,4] on `dev` (the identity for None): ICP updates it in place"""
    if T is None:
        return torch.eye(4, dtype=torch.float64, device=dev)
    return T.detach().to(device=dev, dtype=torch.float64).contiguous().clone()


def sq(distance):
    """float32 square of a distance, as the kernel compares it (+inf stays +inf)"""
    d = torch.tensor(distance, dtype=torch.float32)
    return float(d * d)


def k4(K, what):
    """(fx, fy, cx, cy) from a 3x3 K matrix or four numbers."""
    K = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if K.shape == (3, 3):
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if K.shape == (4,):
        return tuple(float(v) for v in K)
    raise ValueError(f"{what}: expected a 3x3 matrix or (fx, fy, cx, cy), got shape {K.shape}")
