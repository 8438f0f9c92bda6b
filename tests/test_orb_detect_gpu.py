"""gsr_orb_prepare / gsr_orb_detect against the numpy reference (tests/orb_reference.py), bit for bit: the quantised planes with
NaN and out-of-range input, the per-cell slots for per_cell 1 / 4 / 16, corners on cell seams and on the border, the plateau
rule, and run-to-run identity."""
import numpy as np
import pytest
import torch

import orb_reference as R

pytestmark = pytest.mark.gpu
SHAPES = [(96, 64), (70, 45), (35, 35), (34, 40), (32, 200)]      # (W, H): two cells by three with a part cell, one candidate, none


def _image(W, H, seed=0):
    rng = np.random.RandomState(100 + seed)
    g = R.blocky_texture(H, W, seed=W * 1000 + H + seed)
    img = np.stack([g, np.roll(g, 1, axis=1), 0.5 * g + 0.2]).astype(np.float32)
    img += rng.uniform(-0.02, 0.02, size=img.shape).astype(np.float32)
    return img


@pytest.fixture(scope="module")
def cases():
    out = {}
    for W, H in SHAPES:
        img = _image(W, H)
        out[(W, H)] = (img,) + R.prepare_ref(img)
    return out


def _planes(img):
    import scene_utils as su
    u8, box = su.orb_prepare(torch.from_numpy(img).cuda())
    return u8, box


@pytest.mark.parametrize("shape", SHAPES)
def test_planes_bit_for_bit(shape, cases):
    W, H = shape
    img = cases[shape][0].copy()
    rng = np.random.RandomState(7)
    flat = img.reshape(-1)
    where = rng.choice(flat.size, size=24, replace=False)
    flat[where] = np.tile(np.array([np.nan, np.inf, -np.inf, -0.4, 1.3, 3.0e38, 1.0, 0.0], dtype=np.float32), 3)
    u8_ref, box_ref = R.prepare_ref(img)
    u8, box = _planes(img)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W)
    assert np.array_equal(u8.cpu().numpy(), u8_ref)
    assert np.array_equal(box.cpu().numpy().view(np.uint16), box_ref)
    # a single plane is the intensity itself
    g = np.ascontiguousarray(img[0])
    u8_1, box_1 = _planes(g)
    r8, rb = R.prepare_ref(g)
    assert np.array_equal(u8_1.cpu().numpy(), r8) and np.array_equal(box_1.cpu().numpy().view(np.uint16), rb)


@pytest.mark.parametrize("per_cell", [1, 4, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_slots_equal_the_reference(shape, per_cell, cases):
    import scene_utils as su
    W, H = shape
    _, u8_ref, _ = cases[shape]
    ref = R.detect_ref(u8_ref, 20, per_cell)
    u8 = torch.from_numpy(u8_ref).cuda()
    slots = su.orb_detect(u8, 20, per_cell)
    assert tuple(slots.shape) == ref.shape
    assert np.array_equal(slots.cpu().numpy(), ref)
    if min(W, H) < 35:
        assert not ref.any()
    if shape == (96, 64):
        assert (ref[..., 2] > 0).sum() >= 4 * min(per_cell, 2)      # the texture has corners in every inner cell
    again = su.orb_detect(u8, 20, per_cell)
    assert torch.equal(slots, again)      # two runs, the same bits


def test_mask_removes_corners(cases):
    import scene_utils as su
    _, u8_ref, _ = cases[(96, 64)]
    mask = np.ones((64, 96), dtype=np.float32)
    mask[:, 40:60] = 0.0
    ref = R.detect_ref(u8_ref, 20, 4, mask)
    slots = su.orb_detect(torch.from_numpy(u8_ref).cuda(), 20, 4, torch.from_numpy(mask).cuda()).cpu().numpy()
    assert np.array_equal(slots, ref)
    found = slots[slots[..., 2] > 0]
    assert len(found) and not ((found[:, 0] >= 40) & (found[:, 0] < 60)).any()


PLANTED = [(31, 40), (32, 40), (33, 40), (40, 31), (40, 32), (40, 33), (32, 32), (31, 33), (33, 31), (17, 17), (96 - 18, 64 - 18),
           (17, 64 - 18), (96 - 18, 17)]


@pytest.mark.parametrize("at", PLANTED)
def test_a_planted_corner_appears_exactly_once(at):
    import scene_utils as su
    x, y = at
    img = R.plant_corner(np.full((64, 96), 0.3, dtype=np.float32), x, y)
    u8_ref, _ = R.prepare_ref(img)
    ref = R.detect_ref(u8_ref, 20, 4)
    assert ((ref[..., 0] == x) & (ref[..., 1] == y) & (ref[..., 2] > 0)).sum() == 1      # the premise: the tip is a survivor
    u8, _ = _planes(img)
    slots = su.orb_detect(u8, 20, 4).cpu().numpy()
    assert np.array_equal(slots, ref)
    hit = (slots[..., 0] == x) & (slots[..., 1] == y) & (slots[..., 2] > 0)
    assert hit.sum() == 1
    assert slots[hit][0, 2] == ref[(ref[..., 0] == x) & (ref[..., 1] == y) & (ref[..., 2] > 0)][0, 2]
    cell = (y // 32) * 3 + x // 32
    assert hit.reshape(6, 4)[cell].sum() == 1      # ... and in the slots of the cell that owns it


def test_a_plateau_yields_its_raster_first_pixel():
    import scene_utils as su
    # a bright bar two pixels thick ending in the open: its end gives neighbouring pixels of equal score
    img = np.full((64, 96), 0.2, dtype=np.float32)
    img[30:32, 20:50] = 0.8
    u8_ref, _ = R.prepare_ref(img)
    S = R.corner_scores(u8_ref, 20)
    keep = R.nms(S)
    ties = [(y, x) for y, x in zip(*np.nonzero(keep))
            if any(S[y + dy, x + dx] == S[y, x] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))]
    assert ties, "the premise: a survivor with an equal neighbour"
    slots = su.orb_detect(torch.from_numpy(u8_ref).cuda(), 20, 16).cpu().numpy()
    assert np.array_equal(slots, R.detect_ref(u8_ref, 20, 16))
    found = {(int(r[1]), int(r[0])) for r in slots.reshape(-1, 3) if r[2] > 0}
    for y, x in ties:
        assert (y, x) in found
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy, dx) != (0, 0) and S[y + dy, x + dx] == S[y, x]:
                    assert (dy, dx) > (0, 0) and (y + dy, x + dx) not in found      # the equal neighbour comes later, and lost
