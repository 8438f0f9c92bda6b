"""The numpy restatement of k_cam_reduce (tests/helpers.py cam_reduce_*) that tests/test_camera_grad_paths_gpu.py holds the
kernel to bit for bit: it must model the ORDER of the float32 additions, not only their sum."""
import numpy as np

from helpers import CAM_SLOTS, cam_reduce_block, cam_reduce_levels, cam_slots_to_grads


def test_group_order_is_modelled():
    """Rows 0 and 8 fall in group 0, row 1 in group 1: (1e8 + 1) + (-1e8) = 0 in float32, where a row-order sum gives 1."""
    rows = np.zeros((9, CAM_SLOTS), dtype=np.float32)
    rows[0, 0], rows[1, 0], rows[8, 0] = 1e8, -1e8, 1.0
    rows[0, 1], rows[8, 1], rows[1, 1] = 1.0, -1e8, 1e8       # group 0: 1 + (-1e8) = -1e8; + group 1's 1e8 = 0
    rows[1, 2], rows[2, 2], rows[3, 2] = 1e8, 1.0, -1e8       # groups 1, 2, 3 in order: (1e8 + 1) - 1e8 = 0
    t = cam_reduce_block(rows)
    assert t.dtype == np.float32 and t[0] == 0.0 and t[1] == 0.0 and t[2] == 0.0
    naive = np.float32(0)
    for r in range(9):
        naive = np.float32(naive + rows[r, 0])
    assert naive == 1.0                                       # (what an order-blind emulation would give)
    # the eight group sums are added 0 .. 7, not in reverse: groups 5, 6, 7 = 1, 1e8, -1e8
    rows = np.zeros((8, CAM_SLOTS), dtype=np.float32)
    rows[5, 0], rows[6, 0], rows[7, 0] = 1.0, 1e8, -1e8
    assert cam_reduce_block(rows)[0] == 0.0                    # reverse order: (-1e8 + 1e8) + 1 = 1


def test_levels_block_boundaries_and_slot_map():
    """Rows across the 128-row block boundary of the first level: 1e8 in block 0, 1 and -1e8 in block 1 -> level 1 holds
    (1e8, 1 - 1e8 = -1e8), the total 0; with 16 385 rows there are two intermediate levels (129 and 2 rows)."""
    rows = np.zeros((200, CAM_SLOTS), dtype=np.float32)
    rows[0, 5], rows[128, 5], rows[136, 5] = 1e8, 1.0, -1e8
    levels, t = cam_reduce_levels(rows)
    assert len(levels) == 1 and levels[0].shape == (2, CAM_SLOTS)
    assert levels[0][0, 5] == 1e8 and levels[0][1, 5] == -1e8 and t[5] == 0.0
    assert len(cam_reduce_levels(np.zeros((16385, CAM_SLOTS), np.float32))[0]) == 2
    assert [lv.shape[0] for lv in cam_reduce_levels(np.zeros((16385, CAM_SLOTS), np.float32))[0]] == [129, 2]
    assert len(cam_reduce_levels(np.zeros((16384, CAM_SLOTS), np.float32))[0]) == 1
    assert len(cam_reduce_levels(np.zeros((128, CAM_SLOTS), np.float32))[0]) == 0
    _, z = cam_reduce_levels(np.zeros((0, CAM_SLOTS), np.float32))
    assert z.shape == (CAM_SLOTS,) and not z.any()
    dV, dPV, dc = cam_slots_to_grads(np.arange(CAM_SLOTS, dtype=np.float32) + 1)
    assert dV.tolist() == [1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0, 10, 11, 12, 0]
    assert dPV.tolist() == [13, 14, 0, 15, 16, 17, 0, 18, 19, 20, 0, 21, 22, 23, 0, 24]
    assert dc.tolist() == [25, 26, 27]
