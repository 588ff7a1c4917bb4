"""Seeded scenes for the Hamming branch of `reproject_and_match_2d3d` (map points whose observations carry binary
descriptors, a predicted pose, current keypoints + uint8 descriptor rows), in the style of tests/reproject_scenes.py.
Shared by the golden generator (which feeds them to the REFERENCE's function under a cv2 stub) and the tests (which
feed the same arrays to the numpy restatement / the HIP path)."""
import types

import numpy as np

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
W, H = 1241, 376
FLIP = 0.08                                                       # probability of a flipped bit, observation and keypoint rows
CASES = [  # seed, n_pts, n_kp, radius, B (bytes), max_hamm, pix_noise
    (0, 400, 300, 12.0, 32, 64, 2.0), (1, 1500, 1000, 12.0, 32, 64, 2.0), (2, 800, 600, 25.0, 32, 64, 6.0),
    (3, 600, 500, 12.0, 61, 64, 2.0), (4, 50, 40, 3.0, 32, 64, 2.0)]


def noisy(rng, base):
    """`base` (uint8 [..., B]) with each bit flipped with probability FLIP."""
    flips = np.packbits(rng.random(base.shape + (8,)) < FLIP, axis=-1).reshape(base.shape)
    return base ^ flips


def make_case(seed, n_pts, n_kp, radius, B, max_hamm, pix_noise=2.0):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-25, 25, n_pts), rng.uniform(-5, 5, n_pts), rng.uniform(-10, 70, n_pts)], 1)
    ang = rng.uniform(-0.1, 0.1)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    Tcw = np.eye(4)
    Tcw[:3, :3] = R
    Tcw[:3, 3] = rng.normal(0, 0.3, 3)
    Xc = X @ R.T + Tcw[:3, 3]
    proj = (K @ (Xc / Xc[:, 2:3]).T).T[:, :2]
    base = rng.integers(0, 256, (n_pts, B), dtype=np.uint8)
    n_obs = rng.integers(0, 10, n_pts)                            # 0..9 observations, the last six count
    obs_desc, obs_valid = np.zeros((n_pts, 10, B), np.uint8), np.zeros((n_pts, 10), bool)
    for i in range(n_pts):
        for j in range(n_obs[i]):
            if rng.random() < 0.1:                                # an observation stored without descriptor
                continue
            obs_desc[i, j] = noisy(rng, base[i])
            obs_valid[i, j] = True
    vis = np.flatnonzero((Xc[:, 2] > 0.5) & (proj[:, 0] > 0) & (proj[:, 0] < W) & (proj[:, 1] > 0) & (proj[:, 1] < H))
    pick = rng.choice(vis, min(len(vis), n_kp * 2 // 3), replace=False)
    kp = [proj[pick] + rng.normal(0, pix_noise, (len(pick), 2))]
    des = [noisy(rng, base[pick])]
    n_cl = n_kp - len(pick)
    kp.append(np.stack([rng.uniform(0, W, n_cl), rng.uniform(0, H, n_cl)], 1))
    des.append(rng.integers(0, 256, (n_cl, B), dtype=np.uint8))
    kp = np.concatenate(kp).astype(np.float32)
    des = np.ascontiguousarray(np.concatenate(des))
    perm = rng.permutation(len(kp))
    kp, des = kp[perm], np.ascontiguousarray(des[perm])
    ids = rng.permutation(10 * n_pts)[:n_pts]                     # arbitrary, non-contiguous map ids
    wmap = types.SimpleNamespace(points={})
    for i in range(n_pts):
        obs = [(int(j), int(j), obs_desc[i, j].copy() if obs_valid[i, j] else None) for j in range(n_obs[i])]
        wmap.points[int(ids[i])] = types.SimpleNamespace(position=X[i].copy(), observations=obs)
    digest = float(X.sum() + kp.astype(np.float64).sum() + des.astype(np.float64).sum()
                   + obs_desc.astype(np.float64).sum() + ids.sum())
    return dict(wmap=wmap, K=K, Tcw=Tcw, kp=kp, des=des, W=W, H=H, radius=radius, max_hamm=max_hamm, B=B, digest=digest,
                X=X, pick=pick, perm=perm)
