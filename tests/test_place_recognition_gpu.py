"""Place recognition end to end on an analytic textured plane seen from known poses (tests/orb_reference.py plane_view: the
texture is evaluated at the ray-plane hit, the depth is exact): matching quality against the numpy reference on the same keypoints,
the recovered pose against a bound measured on the reference pipeline, the keyframe database's ranking, and a loop-closure edge
that closes a three-node pose graph.

Pose bound (not fixed in advance: keypoints sit on integer pixels, so the error depends on the scene): the reference pipeline -
the same matches, a least-squares (Horn) fit on the pairs whose true reprojection is within 1.5 px - is measured against the known
pose, and relative_pose_from_features may be off by twice that, because its RANSAC inlier set may differ from the reference's by
pairs at the boundary.  Measured values: profiles/orb.txt."""
import numpy as np
import pytest
import torch

import orb_reference as R

pytestmark = pytest.mark.gpu
H, W = 192, 256
K = (260.0, 260.0, 127.5, 95.5)
POSES = [R.pose_w2c(0, 0, 0, [0, 0, 0]), R.pose_w2c(0.03, -0.05, 0.12, [0.08, -0.05, 0.06]),
         R.pose_w2c(-0.04, 0.03, -0.2, [-0.06, 0.04, -0.05]), R.pose_w2c(0.02, 0.06, 0.3, [0.05, 0.06, 0.1])]
REPROJ_PX = 1.5
MD = 0.02      # the correspondence distance in metres: about 2.6 px at the plane's 2 m


def _frame(pose, seed):
    import scene_utils as su
    img, depth = R.plane_view(H, W, K, pose, seed=seed)
    cam = su.camera_from_intrinsics(*K, W, H, w2c=pose, device="cuda")
    return su.Frame(torch.from_numpy(img).cuda(), torch.from_numpy(depth).cuda(), None, cam), img, depth


@pytest.fixture(scope="module")
def scene():
    import scene_utils as su
    out = []
    for i, (pose, seed) in enumerate([(p, 5) for p in POSES] + [(POSES[0], 11), (POSES[0], 12)]):
        frame, img, depth = _frame(pose, seed)
        out.append(dict(frame=frame, img=img, depth=depth, pose=pose, feat=su.detect_orb(frame, levels=1)))
    return out


def _lift(xy, depth):
    u, v = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    z = depth[np.floor(xy[:, 1] + 0.5).astype(int), np.floor(xy[:, 0] + 0.5).astype(int)].astype(np.float64)
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)


def _reprojection_error(a, b, pairs):
    """pixels between keypoint j of b and the true image in b of keypoint i of a"""
    xa, xb = a["feat"].xy.cpu().numpy(), b["feat"].xy.cpu().numpy()
    T = b["pose"] @ np.linalg.inv(a["pose"])
    p = _lift(xa[pairs[:, 0]], a["depth"]) @ T[:3, :3].T + T[:3, 3]
    return np.hypot(K[0] * p[:, 0] / p[:, 2] + K[2] - xb[pairs[:, 1], 0], K[1] * p[:, 1] / p[:, 2] + K[3] - xb[pairs[:, 1], 1])


def _reference_descriptors(s, pattern):
    u8, box = R.prepare_ref(s["img"])
    xy = s["feat"].xy.cpu().numpy()
    kp = np.concatenate([xy.astype(np.int32), s["feat"].score.cpu().numpy()[:, None]], axis=1)
    return R.describe_ref(u8, box, kp, pattern)


def _reference_matches(da, db, md=64, ratio=0.8):
    def passing(q, t):
        i, b, s = R.hamming_ref(q, t)
        return i, (b <= md) & (b.astype(np.float32) < np.float32(ratio) * s.astype(np.float32))
    i, ok = passing(da, db)
    j, ok2 = passing(db, da)
    keep = ok & ok2[i] & (j[i] == np.arange(len(da)))
    return np.stack([np.nonzero(keep)[0], i[keep]], axis=1)


def _pose_error(T, T_true):
    d = np.linalg.inv(T_true) @ T
    return np.linalg.norm(d[:3, 3]), np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))


def test_detection_equals_the_reference_on_the_plane(scene):
    s = scene[0]
    u8, _ = R.prepare_ref(s["img"])
    ref = R.detect_ref(u8, 20, 4).reshape(-1, 3)
    ref = ref[ref[:, 2] > 0]
    f = s["feat"]
    got = np.concatenate([f.xy.cpu().numpy().astype(np.int32), f.score.cpu().numpy()[:, None]], axis=1)
    assert len(got) == len(ref) >= 150 and (f.level.cpu().numpy() == 0).all()
    order = sorted(range(len(ref)), key=lambda r: (-ref[r, 2], ref[r, 1], ref[r, 0]))      # score, then y, x
    assert np.array_equal(got, ref[order])
    assert np.array_equal(f.xy.cpu().numpy(), got[:, :2].astype(np.float32))


def test_matches_reach_the_references_inlier_share_and_the_pose_is_recovered(scene):
    import scene_utils as su
    pattern = R.library_pattern()
    a, b = scene[0], scene[1]
    ra, rb = _reference_descriptors(a, pattern), _reference_descriptors(b, pattern)
    for s, r in ((a, ra), (b, rb)):
        assert (r["margin"] <= 1e-4).mean() <= 0.02
    ref_pairs = _reference_matches(ra["desc"], rb["desc"])
    ref_true = _reprojection_error(a, b, ref_pairs) <= REPROJ_PX
    ref_share = ref_true.mean()
    assert len(ref_pairs) >= 30 and ref_share >= 0.8, (len(ref_pairs), ref_share)
    pairs = su.match_descriptors(a["feat"], b["feat"]).cpu().numpy()
    share = (_reprojection_error(a, b, pairs) <= REPROJ_PX).mean()
    print(f"matches: reference {len(ref_pairs)} with true share {ref_share:.4f}; device {len(pairs)} with true share {share:.4f}")
    assert len(pairs) >= 0.98 * len(ref_pairs) - 1
    assert share >= ref_share - 0.02

    T_true = b["pose"] @ np.linalg.inv(a["pose"])
    xa, xb = a["feat"].xy.cpu().numpy(), b["feat"].xy.cpu().numpy()
    T_ref = R.horn_fit(_lift(xa[ref_pairs[ref_true, 0]], a["depth"]), _lift(xb[ref_pairs[ref_true, 1]], b["depth"]))
    ref_t, ref_r = _pose_error(T_ref, T_true)
    res = su.relative_pose_from_features(a["feat"], a["frame"].depth, a["frame"].camera, b["feat"], b["frame"].depth,
                                         b["frame"].camera, MD, seed=3)
    got_t, got_r = _pose_error(res.transformation.cpu().numpy(), T_true)
    print(f"pose error: reference {ref_t * 1e3:.3f} mm {ref_r:.4f} deg; device {got_t * 1e3:.3f} mm {got_r:.4f} deg; "
          f"fitness {res.fitness:.3f}")
    assert res.converged and res.fitness * len(xa) >= 0.8 * ref_true.sum()
    assert got_t <= 2 * ref_t and got_r <= 2 * ref_r


MIN_VOTES = 20


def test_database_ranks_the_overlapping_views_first(scene):
    import scene_utils as su
    db = su.PlaceDatabase()
    for i in (1, 4, 2, 5, 3):      # overlapping views and unrelated textures, interleaved
        db.add(f"kf{i}", scene[i]["feat"], frame=scene[i]["frame"])
    assert len(db) == 5 and "kf4" in db and db["kf2"].kf_id == "kf2"
    query = scene[0]["feat"]
    votes = dict(zip(["kf1", "kf4", "kf2", "kf5", "kf3"], db.votes(query).tolist()))
    print("votes", votes)
    # the reference on the device's descriptors: the same counts
    desc = [scene[i]["feat"].descriptors.cpu().numpy() for i in (1, 4, 2, 5, 3)]
    seg = np.concatenate([[0], np.cumsum([len(d) for d in desc])])
    assert list(votes.values()) == R.vote_ref(query.descriptors.cpu().numpy(), np.concatenate(desc), seg, 64, 0.8).tolist()
    ranked = db.query(query, top_k=5, min_votes=MIN_VOTES)
    assert {k for k, _ in ranked} == {"kf1", "kf2", "kf3"}
    assert [v for _, v in ranked] == sorted((v for _, v in ranked), reverse=True)
    assert votes["kf4"] < MIN_VOTES and votes["kf5"] < MIN_VOTES
    assert db.query(query, top_k=1, min_votes=MIN_VOTES) == ranked[:1]
    # excluded ids are never returned
    out = db.query(query, exclude=("kf1", "kf3"), top_k=5, min_votes=0)
    assert [k for k, _ in out][0] == "kf2" and not {"kf1", "kf3"} & {k for k, _ in out} and len(out) == 3
    with pytest.raises(ValueError, match="already in the database"):
        db.add("kf1", query)
    # the buffer grows in place: a sixth keyframe, itself
    db.add("kf0", query)
    assert db.query(query, top_k=1, min_votes=MIN_VOTES)[0] == ("kf0", db.votes(query)[5].item())


def test_loop_closure_edge_closes_a_pose_graph(scene):
    import scene_utils as su
    db = su.PlaceDatabase()
    db.add(0, scene[0]["feat"], frame=scene[0]["frame"])
    edge = su.loop_closure_edge(db[0], scene[2]["frame"], features=scene[2]["feat"], max_correspondence_distance=MD, stride=2, seed=1)
    assert edge is not None
    T, info = edge
    T_true = scene[2]["pose"] @ np.linalg.inv(scene[0]["pose"])
    err_t, err_r = _pose_error(T.cpu().numpy(), T_true)
    print(f"loop closure: {err_t * 1e3:.3f} mm {err_r:.4f} deg")
    assert err_t < 0.01 and err_r < 0.3      # ICP on one plane cannot improve the in-plane part: the feature pose's order of size
    assert tuple(info.shape) == (6, 6) and float(info[3, 3]) > 100
    # an unrelated keyframe gives no edge
    db.add(4, scene[4]["feat"], frame=scene[4]["frame"])
    assert su.loop_closure_edge(db[4], scene[2]["frame"], features=scene[2]["feat"], max_correspondence_distance=MD, stride=2, seed=1) is None
    # three keyframes, odometry drifting, the loop closure as the uncertain edge: camera-to-world poses
    c2w = [np.linalg.inv(scene[i]["pose"]) for i in (0, 1, 2)]
    drift = R.pose_w2c(0.0, 0.01, 0.0, [0.01, 0.0, 0.005])
    g = su.PoseGraph()
    g.add_node(c2w[0], fixed=True, id=0)
    g.add_node(c2w[1] @ drift, id=1)
    g.add_node(c2w[2] @ drift @ drift, id=2)
    rel = lambda i, j: np.linalg.inv(c2w[j]) @ c2w[i]      # coordinates of node i in node j
    g.add_edge(0, 1, rel(0, 1))
    g.add_edge(1, 2, rel(1, 2))
    g.add_edge(0, 2, T, info, uncertain=True)
    res = g.optimize(max_correspondence_distance=MD)
    assert res.converged and res.residual_end < res.residual_start
    assert np.linalg.norm(g.pose(2).cpu().numpy()[:3, 3] - c2w[2][:3, 3]) < 0.01
