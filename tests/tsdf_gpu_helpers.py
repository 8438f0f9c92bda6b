"""What the TSDF GPU tests share: frames of tests/tsdf_reference.py on the device, the device volume driven beside the reference
volume (the reference integrates into the blocks the device touched), and the reference volume uploaded."""
import functools

import numpy as np
import torch

import tsdf_reference as R

DEV = "cuda:0"


def camera_of(fr):
    from scene_utils import camera_from_intrinsics
    H, W = fr.depth.shape
    fx, fy, cx, cy = (float(k) for k in fr.K)
    return camera_from_intrinsics(fx, fy, cx, cy, W, H, w2c=fr.w2c, device=DEV)


def on_device(fr):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t(fr.image), t(fr.depth), camera_of(fr), t(fr.mask), torch.from_numpy(fr.w2c)


def new_volume(args):
    from scene_utils import TSDFVolume
    return TSDFVolume(device=DEV, **args)


def integrate_both(vol, ref, fr):
    """one frame into the device volume and, over the blocks the device touched, into the reference; -> the touched keys"""
    image, depth, cam, mask, w2c = on_device(fr)
    keys = vol.touch(depth, cam, mask=mask, w2c=w2c).cpu().numpy()
    vol.integrate(image, depth, cam, mask=mask, w2c=w2c)
    ref.integrate(fr, keys)
    return keys


def run_both(args, frames, shift=None):
    args = dict(args)
    if shift is not None:
        args["origin"] = tuple((np.asarray(args.get("origin", (0.0, 0.0, 0.0))) + np.asarray(shift)).tolist())
        frames = R.shifted(frames, shift)
    vol, ref = new_volume(args), R.RefVolume(**args)
    for fr in frames:
        integrate_both(vol, ref, fr)
    return vol, ref


@functools.lru_cache(maxsize=None)
def scene_pair(name, n_frames=None, shift=None):
    args, frames = R.scenes()[name]
    return run_both(args, frames[:n_frames], shift)


def device_rows(vol, keys):
    """tsdf, weight, color of the device volume as numpy, in the order of `keys`"""
    ks, ros = vol.keys_sorted.cpu().numpy(), vol.row_of_sorted.cpu().numpy()
    rows = ros[np.searchsorted(ks, keys)]
    return vol.tsdf.cpu().numpy()[rows], vol.weight.cpu().numpy()[rows], vol.color.cpu().numpy()[rows]


def uploaded(ref, args):
    """the reference volume rounded to float32 in a device volume: extraction apart from integration"""
    vol = new_volume(args)
    vol.load(ref.keys, ref.tsdf.astype(np.float32), ref.weight.astype(np.float32), ref.color.astype(np.float32))
    return vol
