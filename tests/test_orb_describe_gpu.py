"""gsr_orb_describe against the numpy reference: the moments as integers, the orientation bin and the 256 bits wherever the
reference's float64 angle lies further than 1e-4 rad from a bin boundary (at most 2 % of the keypoints may be excluded so, which
is checked on the reference alone), skipped rows, and the exact quarter turn."""
import numpy as np
import pytest
import torch

import orb_reference as R

pytestmark = pytest.mark.gpu
SHAPES = [(96, 64), (70, 45), (35, 35), (34, 40), (32, 200)]
SEEDS = {(96, 64): 2, (70, 45): 5, (35, 35): 1, (34, 40): 0, (32, 200): 0}      # textures whose angles stay off the boundaries
MARGIN = 1e-4


def _case(W, H):
    img = R.blocky_texture(H, W, seed=SEEDS[(W, H)], block=4)
    u8, box = R.prepare_ref(img)
    if min(W, H) >= 35:      # every pixel that qualifies, as a keypoint - corner or not
        ys, xs = np.mgrid[R.BORDER:H - R.BORDER:3, R.BORDER:W - R.BORDER:3]
        kp = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 30)], axis=1).astype(np.int32)
    else:
        kp = np.zeros((0, 3), dtype=np.int32)
    # rows the kernel must skip: an empty slot, and keypoints inside the border or outside the image
    skipped = np.array([[0, 0, 0], [W // 2, H // 2, 0], [16, H // 2, 9], [W - 17, H // 2, 9], [W // 2, 16, 9], [W // 2, H - 17, 9],
                        [-5, 3, 9], [W + 40, H + 40, 9]], dtype=np.int32)
    return img, u8, box, np.concatenate([kp, skipped])


def _describe(u8, box, kp):
    import scene_utils as su
    b, d, m = su.orb_describe(torch.from_numpy(u8).cuda(), torch.from_numpy(box.view(np.int16)).cuda(), torch.from_numpy(kp).cuda(),
                              return_moments=True)
    return b.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy()


@pytest.fixture(scope="module")
def pattern():
    return R.library_pattern()


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_bins_and_bits(shape, pattern):
    W, H = shape
    _, u8, box, kp = _case(W, H)
    ref = R.describe_ref(u8, box, kp, pattern)
    live = ref["bin"] >= 0
    assert live.sum() == len(kp) - 8
    decided = ref["margin"] > MARGIN
    if live.any():
        assert (~decided[live]).mean() <= 0.02, "choose another seed: the reference itself is undecided too often"
    bins, desc, mom = _describe(u8, box, kp)
    assert np.array_equal(mom, ref["moments"])
    assert np.array_equal(bins[~live], np.full((~live).sum(), -1)) and not desc[~live].any()
    assert np.array_equal(bins[decided], ref["bin"][decided])
    assert np.array_equal(desc[decided], ref["desc"][decided])
    assert ((bins[live] >= 0) & (bins[live] < 30)).all()
    again = _describe(u8, box, kp)
    assert all(np.array_equal(a, b) for a, b in zip((bins, desc, mom), again))
    if shape == (96, 64):
        assert len(np.unique(ref["bin"][live])) >= 15 and len(np.unique(desc[live], axis=0)) > 0.9 * live.sum()


def test_zero_keypoints_is_legal():
    import scene_utils as su
    u8 = torch.zeros((40, 40), dtype=torch.uint8, device="cuda")
    b, d = su.orb_describe(u8, torch.zeros((40, 40), dtype=torch.int16, device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert tuple(b.shape) == (0,) and tuple(d.shape) == (0, 8)


def test_a_quarter_turn_moves_every_decided_bin_by_7_or_8(pattern):
    import scene_utils as su
    W, H = 96, 64
    img, u8, box, kp = _case(W, H)
    kp = kp[:-8]
    rot = np.ascontiguousarray(np.rot90(img))      # [W, H]: (x, y) -> (y, W - 1 - x)
    u8r, boxr = su.orb_prepare(torch.from_numpy(rot).cuda())
    assert np.array_equal(u8r.cpu().numpy(), np.rot90(u8)) and np.array_equal(boxr.cpu().numpy().view(np.uint16), np.rot90(box))
    kpr = np.stack([kp[:, 1], W - 1 - kp[:, 0], kp[:, 2]], axis=1).astype(np.int32)
    inside = (kpr[:, 0] >= R.BORDER) & (kpr[:, 0] < H - R.BORDER) & (kpr[:, 1] >= R.BORDER) & (kpr[:, 1] < W - R.BORDER)
    assert inside.all()
    b0, _, m0 = _describe(u8, box, kp)
    b1, _, m1 = _describe(np.ascontiguousarray(np.rot90(u8)), np.ascontiguousarray(np.rot90(box)), kpr)
    assert np.array_equal(m1[:, 0], m0[:, 1]) and np.array_equal(m1[:, 1], -m0[:, 0])      # dx' = dy, dy' = -dx
    ref0 = R.describe_ref(u8, box, kp, pattern)
    ref1 = R.describe_ref(np.rot90(u8), np.rot90(box), kpr, pattern)
    decided = (ref0["margin"] > MARGIN) & (ref1["margin"] > MARGIN)
    assert decided.mean() >= 0.96
    moved = (b0[decided] - b1[decided]) % 30      # the angle falls by 90 degrees = 7.5 bins
    assert np.isin(moved, (7, 8)).all() and (moved == 7).any() and (moved == 8).any()
