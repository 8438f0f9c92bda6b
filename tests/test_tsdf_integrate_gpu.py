"""gsr_tsdf_touch and gsr_tsdf_integrate against the float64 reference (tests/tsdf_reference.py): the touched set between the
reference's must and may sets, values on decided voxels within their float32 bounds, exact weights, append-only storage."""
import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu


def H():
    import tsdf_gpu_helpers
    return tsdf_gpu_helpers


def check_values(vol, ref, what):
    t, w, c = H().device_rows(vol, ref.keys)
    sure = ~ref.undecided
    assert np.array_equal(w[sure], ref.weight[sure]), what
    et = np.abs(t - ref.tsdf)
    ec = np.abs(c - ref.color).max(axis=-1)
    # float32 storage of the running average is inside the bound's three roundings per update
    rt = (et[sure] / np.maximum(ref.err[sure], 1e-30))[ref.weight[sure] > 0]
    rc = (ec[sure] / np.maximum(ref.err_color[sure], 1e-30))[ref.weight[sure] > 0]
    print(f"{what}: {len(ref.keys)} blocks, undecided {ref.undecided.mean():.2e}, error / bound: tsdf {rt.max(initial=0):.3f}, "
          f"colour {rc.max(initial=0):.3f}")
    assert np.all(et[sure] <= ref.err[sure]), what
    assert np.all(ec[sure] <= ref.err_color[sure]), what
    unseen = sure & (ref.weight == 0)
    assert np.all(t[unseen] == 0) and np.all(c[unseen] == 0)


@pytest.mark.parametrize("name", ["plane", "sphere"])
def test_touch_between_must_and_may(name):
    args, frames = R.scenes()[name]
    vol, ref = H().new_volume(args), R.RefVolume(**args)
    for fr in frames[:3]:
        image, depth, cam, mask, w2c = H().on_device(fr)
        got = set(vol.touch(depth, cam, mask=mask, w2c=w2c).cpu().numpy().tolist())
        must, may, _ = ref.touch(fr)
        assert set(must.tolist()) <= got <= set(may.tolist())
        assert len(got) > 10
    assert vol.num_blocks == 0                       # touch allocates nothing


@pytest.mark.parametrize("name,n", [("plane", 1), ("plane", 8), ("sphere", 12), ("near", 2), ("half_mask", 2), ("one_block", 1)])
def test_values_within_bounds(name, n):
    vol, ref = H().scene_pair(name, n)
    check_values(vol, ref, f"{name} after {n}")
    ks = vol.keys_sorted.cpu().numpy()
    assert np.all(np.diff(ks) > 0)
    assert np.array_equal(np.sort(vol.row_of_sorted.cpu().numpy()), np.arange(vol.num_blocks))
    assert np.array_equal(np.sort(ref.keys), ks)
    assert np.array_equal(vol.block_coords().cpu().numpy(), R.key_block(ks))
    if name == "plane":
        assert (R.key_block(ks).min(axis=0) < 0).all()          # negative block coordinates on every axis
    if name == "one_block":
        assert vol.num_blocks == 1
    if name == "near":
        args, frames = R.scenes()[name]
        g = 8 * R.key_block(ref.keys)[:, None, :] + R.local_coords()[None]
        z = args["origin"][2] + (g[..., 2] + 0.5) * args["voxel_size"]
        assert (z < 0).any() and (ref.weight[z < 0] == 0).all()       # voxels behind the camera stay untouched
        assert ((ref.weight == 0) & (z > 0)).any()                    # and some in front project outside the image


def test_max_weight_cap_is_reached():
    vol, ref = H().scene_pair("capped")
    check_values(vol, ref, "capped")
    assert float(vol.weight.max()) == 3.0 and (vol.weight == 3.0).sum() > 1000


def test_far_from_the_origin_keeps_the_bounds():
    near, ref_near = H().scene_pair("plane", 2)
    far, ref_far = H().scene_pair("plane", 2, R.FAR_SHIFT)
    check_values(far, ref_far, "plane shifted 10 km")
    assert ref_far.err.max() <= 1.001 * ref_near.err.max() + 1e-12
    assert np.array_equal(np.sort(ref_far.keys), np.sort(ref_near.keys))


def test_second_frame_leaves_untouched_rows_alone():
    args, frames = R.scenes()["sphere"]
    vol, ref = H().new_volume(args), R.RefVolume(**args)
    H().integrate_both(vol, ref, frames[0])
    B0 = vol.num_blocks
    keys0 = vol.keys_sorted.clone()
    rows0 = vol.row_of_sorted.clone()
    before = (vol.tsdf.clone(), vol.weight.clone(), vol.color.clone())
    touched = H().integrate_both(vol, ref, frames[5])
    assert vol.num_blocks > B0                                   # the frame added blocks
    # rows keep their place: the old keys still name the old rows
    pos = torch.searchsorted(vol.keys_sorted, keys0)
    assert torch.equal(vol.row_of_sorted[pos], rows0)
    ks, ros = keys0.cpu().numpy(), rows0.cpu().numpy()
    untouched = torch.from_numpy(ros[~np.isin(ks, touched)]).long().to(vol.device)
    assert len(untouched) > 0
    for old, new in zip(before, (vol.tsdf, vol.weight, vol.color)):
        assert torch.equal(old[untouched].view(torch.int32), new[untouched].view(torch.int32))
    check_values(vol, ref, "two frames")


def test_all_zero_depth_gives_an_empty_volume():
    args, frames = R.scenes()["plane"]
    vol = H().new_volume(args)
    image, depth, cam, mask, w2c = H().on_device(frames[0])
    assert vol.integrate(image, torch.zeros_like(depth), cam, w2c=w2c) == 0
    assert vol.num_blocks == 0 and vol.block_coords().shape == (0, 3)
    p, n, c = vol.extract_point_cloud()
    assert p.shape == n.shape == c.shape == (0, 3)
    v, t, c = vol.extract_triangle_mesh()
    assert v.shape == (0, 3) and t.shape == (0, 3) and t.dtype == torch.int64 and c.shape == (0, 3)
    s, _, sc = vol.extract_triangle_mesh(weld=False)
    assert s.shape == (0, 3, 3) and sc.shape == (0, 3, 3)
    torch.cuda.synchronize()


def test_frame_form_and_repeatability():
    from scene_utils import Frame
    args, frames = R.scenes()["plane"]
    runs = []
    for _ in range(2):
        vol = H().new_volume(args)
        for fr in frames[:3]:
            image, depth, cam, mask, w2c = H().on_device(fr)
            vol.integrate(Frame(image, depth, mask, cam), w2c=w2c)
        runs.append(vol)
    a, b = runs
    assert torch.equal(a.keys_sorted, b.keys_sorted) and torch.equal(a.row_of_sorted, b.row_of_sorted)
    for x, y in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.color, b.color)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ref = H().scene_pair("plane", 3)[0]
    assert torch.equal(a.tsdf.view(torch.int32), ref.tsdf.view(torch.int32))     # the Frame form is the tensor form
    vol.reset()
    assert vol.num_blocks == 0


def test_cpu_tensors_and_bad_library_arguments_are_refused():
    import ctypes as C
    from diff_gaussian_rasterization import _C
    args, frames = R.scenes()["plane"]
    vol = H().new_volume(args)
    image, depth, cam, mask, w2c = H().on_device(frames[0])
    with pytest.raises(_C.GsrError, match="no CPU path"):
        vol.integrate(image, depth.cpu(), cam)
    with pytest.raises(ValueError):
        vol.integrate(image, depth[:-1], cam)
    with pytest.raises(ValueError):
        vol.extract_point_cloud(min_weight=-1)
    bad = _C.gsr_tsdf_volume((C.c_double * 3)(0, 0, 0), 0.1, 0.05, 1.0, 1.0, 0.0)          # sdf_trunc < voxel_size
    count = torch.zeros(1, dtype=torch.int64, device=vol.device)
    assert _C.lib().gsr_tsdf_extract_points(C.byref(bad), 0, *([None] * 5), 0.0, 0, None, None, None, _C.ptr(count), None, 0,
                                            None) == -1
    assert "sdf_trunc" in _C.last_error()
    assert _C.lib().gsr_tsdf_extract_triangles(C.byref(vol._vol()), -1, *([None] * 5), 0.0, 0, None, None, _C.ptr(count), None, 0,
                                               None) == -1
    assert vol.num_blocks == 0
