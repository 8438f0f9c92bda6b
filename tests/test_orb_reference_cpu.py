"""CPU tests of the sparse-feature front end: the numpy reference on hand-built cases, the sampling pattern the library was built
with against tools/make_orb_pattern.py, and the argument checks of every new function (nothing here needs a device)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import orb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arc_case(n_bright, centre=100, ring=160, rest=100):
    """a 7 x 7 patch: centre pixel `centre`, the first n circle pixels `ring`, the others `rest`"""
    u8 = np.full((7, 7), rest, dtype=np.uint8)
    u8[3, 3] = centre
    for dx, dy in R.CIRCLE[:n_bright]:
        u8[3 + dy, 3 + dx] = ring
    return u8


def test_bright_arc_of_nine_is_a_corner_and_of_eight_is_not():
    assert R.fast_score_at(_arc_case(9), 3, 3) == 60
    assert R.fast_score_at(_arc_case(8), 3, 3) == 0
    assert R.fast_score_at(_arc_case(16), 3, 3) == 60


def test_dark_arc_and_the_weakest_pixel_sets_the_score():
    assert R.fast_score_at(_arc_case(9, centre=200, ring=50, rest=200), 3, 3) == 150
    u8 = _arc_case(9)
    dx, dy = R.CIRCLE[4]
    u8[3 + dy, 3 + dx] = 130      # one weaker pixel inside the arc
    assert R.fast_score_at(u8, 3, 3) == 30


def test_vectorised_scores_equal_the_per_pixel_rule():
    u8, _ = R.prepare_ref(R.blocky_texture(45, 50, seed=3))
    S = R.corner_scores(u8, 20)
    for y in range(R.BORDER, 45 - R.BORDER):
        for x in range(R.BORDER, 50 - R.BORDER):
            s = R.fast_score_at(u8, x, y)
            assert S[y, x] == (s if s > 20 else 0)
    assert not S[:R.BORDER].any() and not S[:, :R.BORDER].any() and not S[45 - R.BORDER:].any()


def test_nms_tie_rule_keeps_the_raster_first_pixel():
    S = np.zeros((6, 6), dtype=np.int64)
    S[2, 2] = S[2, 3] = S[3, 1] = 40      # a plateau: (2,2) comes first in raster order
    S[4, 4] = 50
    S[4, 5] = 49
    keep = R.nms(S)
    assert sorted(zip(*np.nonzero(keep))) == [(2, 2), (4, 4)]


def test_prepare_rule_on_special_values():
    I = np.array([[0.0, 1.0, np.nan, np.inf, -np.inf, -0.3, 1.7, 0.5, 1.0 / 255.0, 0.4999 / 255.0]], dtype=np.float32)
    u8, box = R.prepare_ref(I)
    assert u8.tolist() == [[0, 255, 0, 255, 0, 0, 255, 128, 1, 0]]
    assert int(box[0, 0]) == 5 * (3 * 0 + 255 + 0) and box.dtype == np.uint16


def _tool():
    spec = importlib.util.spec_from_file_location("make_orb_pattern", os.path.join(ROOT, "tools", "make_orb_pattern.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_pattern_is_the_tools_pattern_and_stays_inside_the_disc():
    pat = R.library_pattern()
    assert pat.shape == (30, 256, 4) and pat.dtype == np.int8
    assert pat.tobytes() == _tool().pattern_bytes()
    p = pat.astype(np.int64)
    assert (p[..., 0] ** 2 + p[..., 1] ** 2).max() <= 225 and (p[..., 2] ** 2 + p[..., 3] ** 2).max() <= 225
    # bin k is bin 0 turned by 12 k degrees, up to the rounding
    a = 2 * np.pi * 7 / 30
    turned = np.stack([p[0, :, 0] * np.cos(a) - p[0, :, 1] * np.sin(a), p[0, :, 0] * np.sin(a) + p[0, :, 1] * np.cos(a)], axis=1)
    assert np.abs(turned - p[7, :, :2]).max() <= 1.5


def test_hamming_of_known_words():
    q = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0x0F]], dtype=np.int32)
    db = np.array([[-1, -1, -1, -1, -1, -1, -1, -1], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert R.hamming_matrix(q, db).tolist() == [[256, 1, 1], [220, 35, 35]]
    idx, best, second = R.hamming_ref(q, db)
    assert idx.tolist() == [1, 1] and best.tolist() == [1, 35] and second.tolist() == [1, 35]
    idx, best, second = R.hamming_ref(q, db[:1])
    assert idx.tolist() == [0, 0] and second.tolist() == [R.NONE, R.NONE]
    idx, best, second = R.hamming_ref(q, db[:0])
    assert idx.tolist() == [-1, -1] and best.tolist() == [R.NONE, R.NONE]
    assert R.vote_ref(q, db, [0, 0, 1, 3], 64, 0.8).tolist() == [0, 0, 0]      # 1 < 0.8 * 1 fails: a duplicated best
    assert R.vote_ref(q, db, [0, 0, 2, 3], 64, 0.8).tolist() == [0, 2, 2]


def test_horn_fit_recovers_a_pose():
    rng = np.random.RandomState(0)
    src = rng.randn(20, 3)
    T = R.pose_w2c(0.1, -0.2, 0.3, [0.1, 0.2, -0.3])
    dst = src @ T[:3, :3].T + T[:3, 3]
    assert np.abs(R.horn_fit(src, dst) - T).max() < 1e-12


def test_plane_view_depth_is_the_ray_plane_hit():
    K = (120.0, 120.0, 47.5, 31.5)
    T = R.pose_w2c(0.05, -0.04, 0.02, [0.03, -0.02, 0.1])
    img, depth = R.plane_view(64, 96, K, T, seed=1)
    assert img.shape == (3, 64, 96) and depth.shape == (64, 96)
    u, v = 70, 20
    pc = np.array([(u - K[2]) / K[0], (v - K[3]) / K[1], 1.0]) * depth[v, u]
    pw = T[:3, :3].T @ (pc - T[:3, 3])
    assert abs(pw[2] - 2.0) < 1e-5


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks_of_the_image_functions():
    import scene_utils as su
    from diff_gaussian_rasterization import _C
    img = torch.zeros(3, 40, 40)
    with pytest.raises(ValueError, match="image: expected a floating-point tensor of shape"):
        su.detect_orb(torch.zeros(2, 40, 40))
    with pytest.raises(_C.GsrError, match="image must live on the HIP device"):
        su.detect_orb(img)
    with pytest.raises(ValueError, match="levels=5: expected 1 .. 4"):
        su.detect_orb(img, levels=5)
    with pytest.raises(TypeError, match="threshold=2.5: expected an int"):
        su.detect_orb(img, threshold=2.5)
    with pytest.raises(ValueError, match="per_cell=17: expected 1 .. 16"):
        su.detect_orb(img, per_cell=17)
    with pytest.raises(ValueError, match="max_keypoints=0"):
        su.detect_orb(img, max_keypoints=0)
    with pytest.raises(ValueError, match="mask: expected a floating-point tensor of shape \\(40, 40\\)"):
        su.detect_orb(img, mask=torch.zeros(3, 3))
    with pytest.raises(_C.GsrError, match="image must live on the HIP device"):
        su.orb_prepare(img)
    with pytest.raises(ValueError, match="u8: expected a uint8 tensor"):
        su.orb_detect(torch.zeros(4, 4))
    with pytest.raises(_C.GsrError, match="u8 must live on the HIP device"):
        su.orb_detect(torch.zeros(40, 40, dtype=torch.uint8))
    with pytest.raises(ValueError, match="threshold=255: expected 0 .. 254"):
        su.orb_detect(torch.zeros(40, 40, dtype=torch.uint8), threshold=255)
    with pytest.raises(ValueError, match="keypoints: expected an int32 tensor of shape \\(M, 3\\)"):
        su.orb_describe(torch.zeros(40, 40, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.int16), torch.zeros(2, 2))
    with pytest.raises(ValueError, match="box: expected \\(40, 40\\) like u8"):
        su.orb_describe(torch.zeros(40, 40, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.int16),
                        torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(_C.GsrError, match="orb_describe needs its tensors on the HIP device"):
        su.orb_describe(torch.zeros(40, 40, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.int16),
                        torch.zeros(2, 3, dtype=torch.int32))


def _features(n=3):
    import scene_utils as su
    z = torch.zeros(n, dtype=torch.int32)
    return su.OrbFeatures(torch.zeros(n, 2), z, z, z, torch.zeros(n, 8, dtype=torch.int32))


def test_argument_checks_of_matching_and_lifting():
    import scene_utils as su
    from diff_gaussian_rasterization import _C
    d = torch.zeros(3, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="a: expected an int32 tensor of shape \\(N, 8\\)"):
        su.match_descriptors(torch.zeros(3, 8), d)
    with pytest.raises(ValueError, match="b: expected an int32 tensor of shape \\(N, 8\\)"):
        su.match_descriptors(d, torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(_C.GsrError, match="a must live on the HIP device"):
        su.match_descriptors(_features(), d)
    with pytest.raises(ValueError, match="max_distance=300: expected 0 .. 256"):
        su.match_descriptors(d, d, max_distance=300)
    with pytest.raises(ValueError, match="ratio=1.5: expected 0 .. 1.0"):
        su.match_descriptors(d, d, ratio=1.5)
    with pytest.raises(TypeError, match="mutual=1: expected a bool"):
        su.match_descriptors(d, d, mutual=1)
    with pytest.raises(_C.GsrError, match="query must live on the HIP device"):
        su.hamming_match(d, d)
    cam = su.camera_from_intrinsics(50.0, 50.0, 19.5, 14.5, 40, 30)
    with pytest.raises(TypeError, match="features: expected OrbFeatures"):
        su.keypoint_points(d, torch.zeros(30, 40), cam)
    with pytest.raises(ValueError, match="depth: expected a floating-point tensor of shape \\(30, 40\\)"):
        su.keypoint_points(_features(), torch.zeros(40, 30), cam)
    with pytest.raises(ValueError, match="max_depth=0.5: expected a value > min_depth=1.0"):
        su.keypoint_points(_features(), torch.zeros(30, 40), cam, min_depth=1.0, max_depth=0.5)
    with pytest.raises(_C.GsrError, match="depth must live on the HIP device"):
        su.keypoint_points(_features(), torch.zeros(30, 40), cam)
    with pytest.raises(ValueError, match="max_correspondence_distance=-1"):
        su.relative_pose_from_features(_features(), None, cam, _features(), None, cam, -1)


def test_argument_checks_of_the_database_and_the_edge():
    import scene_utils as su
    from diff_gaussian_rasterization import _C
    db = su.PlaceDatabase(device="cpu")
    assert len(db) == 0 and 3 not in db
    with pytest.raises(ValueError, match="ratio=-0.1"):
        su.PlaceDatabase(device="cpu", ratio=-0.1)
    with pytest.raises(TypeError, match="features: expected OrbFeatures"):
        db.add(0, torch.zeros(3, 8, dtype=torch.int32))
    with pytest.raises(_C.GsrError, match="features.descriptors must live on the HIP device"):
        db.add(0, _features())
    with pytest.raises(ValueError, match="top_k=0"):
        db.query(_features(), top_k=0)
    with pytest.raises(TypeError, match="min_votes=1.5: expected an int"):
        db.query(_features(), min_votes=1.5)
    cam = su.camera_from_intrinsics(50.0, 50.0, 19.5, 14.5, 40, 30)
    frame = su.Frame(torch.zeros(3, 30, 40), torch.ones(30, 40), None, cam)
    with pytest.raises(ValueError, match="db_entry: expected a PlaceEntry that holds its frame"):
        su.loop_closure_edge(su.PlaceEntry(0, _features(), None), frame)
    entry = su.PlaceEntry(0, _features(), frame)
    with pytest.raises(ValueError, match="frame: expected a Frame with depth"):
        su.loop_closure_edge(entry, su.Frame(torch.zeros(3, 30, 40), None, None, cam))
    with pytest.raises(ValueError, match="min_fitness=2: expected 0 .. 1.0"):
        su.loop_closure_edge(entry, frame, features=_features(), min_fitness=2)
    with pytest.raises(ValueError, match="stride=0"):
        su.loop_closure_edge(entry, frame, features=_features(), stride=0)


def test_library_rejects_bad_arguments_before_any_launch():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    assert lib.gsr_orb_cells(96, 64) == 6 and lib.gsr_orb_cells(70, 45) == 6 and lib.gsr_orb_cells(0, 5) == 0
    assert lib.gsr_orb_prepare(0, 4, None, 3, None, None, None) == -1
    assert lib.gsr_orb_prepare(4, 4, 16, 2, 16, 16, None) == -1
    assert lib.gsr_orb_detect(40, 40, 16, None, 255, 4, 16, None) == -1
    assert lib.gsr_orb_detect(40, 40, 16, None, 20, 17, 16, None) == -1
    assert lib.gsr_orb_describe(40, 40, 16, 16, 3, None, None, None, None, None) == -1
    assert lib.gsr_orb_describe(40, 40, 16, 16, 0, None, None, None, None, None) == 0
    assert lib.gsr_orb_pattern(None) == -1
    assert lib.gsr_hamming_match(3, None, 0, None, 16, 16, 16, None) == -1
    assert lib.gsr_hamming_match(3, 24, 0, None, 16, 16, 16, None) == -1      # a misaligned query
    assert lib.gsr_hamming_match(0, None, 0, None, None, None, None, None) == 0
    assert lib.gsr_hamming_vote(0, None, 0, None, 70000, 16, 64, 0.8, 16, None) == -1
    assert lib.gsr_hamming_vote(0, None, 0, None, 1, 16, 64, float("nan"), 16, None) == -1
    assert lib.gsr_hamming_vote(0, None, 0, None, 0, None, 64, 0.8, None, None) == 0
