"""numpy restatement of the Hamming branch of the reference's `reproject_and_match_2d3d` (slam/core/pnp_utils.py:224-304
with `des_cur.dtype == np.uint8`: `_desc_distance` :78-112 takes cv2.norm(a, b, NORM_HAMMING) = popcount(a ^ b), the
threshold is `max_hamm`), with the tie rule this backend DEFINES: among equal minima the lowest keypoint index wins.

The reference takes the first candidate with `d < best_d` in the order `cKDTree.query_ball_point` returns, which for one
query point is the tree's traversal order; so the two can differ only on a decision that is accepted
(`best_d <= max_hamm`) AND tied at the minimum.  `ties` counts exactly those decisions: where it is 0 (every scene of
tests/golden/reproject_hamming.npz, asserted by its generator) this restatement and the reference agree whatever the
traversal order.

Everything else as the float restatement (oracle/reproject_ref.py): brute-force radius search (squared distance in
float64 <= r^2), a point whose LAST observation has no descriptor is skipped, the minimum runs over the last six
observations that have a uint8 descriptor of the frame's width (another dtype or width scores inf), greedy in
`world_map.points` order, `best_d == max_hamm` is accepted."""
import numpy as np

POPCOUNT = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def project_points(K, Tcw, pts_w):
    """`_project_points` (:130-144): float64 camera coordinates, float32 pixels, -1 where z <= 1e-8."""
    pts_w = np.asarray(pts_w, np.float64)
    Xc = pts_w @ Tcw[:3, :3].T + Tcw[:3, 3]
    z = Xc[:, 2]
    uv = np.full((len(pts_w), 2), -1.0, np.float32)
    valid = z > 1e-8
    if np.any(valid):
        proj = (K @ (Xc[valid] / z[valid, None]).T).T
        uv[valid] = proj[:, :2].astype(np.float32, copy=False)
    return uv, z


def hamming_rows(obs, rows):
    """[len(obs), len(rows)] popcount(obs_j ^ rows_i)."""
    return POPCOUNT[obs[:, None, :] ^ rows[None, :, :]].sum(-1)


def reproject_and_match_hamming(world_map, K, Tcw_pred, kps_cur, des_cur, img_w, img_h, radius_px=12.0, max_hamm=64):
    """-> (pts3d f32 [M,3], pts2d f32 [M,2], kp_indices, mp_ids, ties, decisions): `ties` = accepted decisions whose
    minimum was shared by more than one free keypoint; `decisions` = [(mp_id, kp index, distance)] of the accepted."""
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), [], [], 0, [])
    if des_cur is None or len(des_cur) == 0 or not world_map.points:
        return empty
    pts2d = np.asarray(kps_cur, np.float32).reshape(-1, 2)
    if len(pts2d) == 0:
        return empty
    des_cur = np.asarray(des_cur)
    assert des_cur.dtype == np.uint8, "float descriptors: oracle/reproject_ref.py"
    des_cur = des_cur.reshape(len(pts2d), -1)
    B = des_cur.shape[1]
    items = list(world_map.points.items())
    pts3d_all = np.asarray([mp.position for _, mp in items], np.float64)
    uv_all, z_all = project_points(np.asarray(K, np.float64), np.asarray(Tcw_pred, np.float64), pts3d_all)
    cand = np.flatnonzero((z_all > 0.0) & (uv_all[:, 0] >= 0.0) & (uv_all[:, 0] < float(img_w))
                          & (uv_all[:, 1] >= 0.0) & (uv_all[:, 1] < float(img_h)))
    kp64 = pts2d.astype(np.float64)
    used = np.zeros(len(pts2d), bool)
    out3, out2, kpids, mpids, decisions = [], [], [], [], []
    ties = 0
    r2 = float(radius_px) ** 2
    for a in cand:
        mp_id, mp = items[a]
        d2 = np.sum((kp64 - uv_all[a].astype(np.float64)) ** 2, axis=1)
        near = np.flatnonzero(d2 <= r2)
        if len(near) == 0 or not mp.observations or mp.observations[-1][2] is None:
            continue
        obs = [np.asarray(d).reshape(-1) for _, _, d in mp.observations[-6:] if d is not None]
        obs = [d for d in obs if d.dtype == np.uint8 and d.shape[0] == B]
        free = near[~used[near]]                                # ascending keypoint index
        if len(obs) == 0 or len(free) == 0:
            continue                                            # (every distance inf: `d < 1e9` never holds)
        d = hamming_rows(np.stack(obs), des_cur[free]).min(0)
        best_d = int(d.min())
        if best_d > max_hamm:
            continue
        best_i = int(free[int(np.argmax(d == best_d))])         # the lowest index among the equal minima
        ties += int((d == best_d).sum() > 1)
        used[best_i] = True
        out3.append(pts3d_all[a].astype(np.float32)); out2.append(pts2d[best_i]); kpids.append(best_i); mpids.append(mp_id)
        decisions.append((mp_id, best_i, best_d))
    if not out3:
        return empty
    return np.asarray(out3, np.float32), np.asarray(out2, np.float32), kpids, mpids, ties, decisions
