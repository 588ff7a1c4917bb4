"""Seeded 2D-3D scenes for `solve_pnp_ransac` / `refine_pose_pnp`: a world->camera pose, map points in front of the
camera, their projections with 0.5 px of noise, and a chosen fraction of outliers (pixels drawn anywhere in the image).

Two cameras: KITTI's (tests/reproject_scenes.py, 1241 x 376; points 4 - 60 m ahead, as the tracker sees them) and the
reference test's random-pose camera (fx 450, fy 460, 640 x 480 image; points 2 - 8 m ahead, rotation up to 0.3 rad about
a random axis, slam/core tests/test_pnp_utils.py)."""
import numpy as np

from reproject_scenes import H as KITTI_H, K as KITTI_K, W as KITTI_W

K_RAND = np.array([[450.0, 0, 300.0], [0, 460.0, 200.0], [0, 0, 1.0]])
RAND_W, RAND_H = 640, 480
NOISE_PX = 0.5
RANSAC_PX, CONF, ITERS = 2.5, 0.999, 300


def random_rotation(rng, max_angle=0.3):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def make_scene(seed, n, outlier_frac, camera="kitti", noise_px=NOISE_PX):
    """Returns dict(pts3d f32 [n,3], pts2d f32 [n,2], K, Tcw (ground truth), inlier bool [n])."""
    rng = np.random.default_rng(seed)
    if camera == "kitti":
        K, W, H, zr = KITTI_K, KITTI_W, KITTI_H, (4.0, 60.0)
        R = random_rotation(rng, 0.1)
        t = rng.normal(0, 0.3, 3)
    else:
        K, W, H, zr = K_RAND, RAND_W, RAND_H, (2.0, 8.0)
        R = random_rotation(rng, 0.3)
        t = rng.normal(0, 0.5, 3)
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = R, t
    # points drawn in the camera frame (inside the image), then taken to the world frame
    u = rng.uniform(0, W, n)
    v = rng.uniform(0, H, n)
    z = rng.uniform(*zr, n)
    Xc = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)
    Xw = (Xc - t) @ R
    proj = np.stack([u, v], 1) + rng.normal(0, noise_px, (n, 2)) if noise_px else np.stack([u, v], 1)
    n_out = int(round(outlier_frac * n))
    out = rng.choice(n, n_out, replace=False)
    proj[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], 1)
    inlier = np.ones(n, bool)
    inlier[out] = False
    return dict(pts3d=Xw.astype(np.float32), pts2d=proj.astype(np.float32), K=K.copy(), Tcw=Tcw, inlier=inlier)


def rot_err_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.degrees(np.arccos(max(-1.0, min(1.0, c)))))


def rot_err_rad(Ra, Rb):
    """Angle of Ra^T Rb, accurate for small angles (from the skew part)."""
    D = Ra.T @ Rb
    w = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) * 0.5
    return float(np.arctan2(np.linalg.norm(w), (np.trace(D) - 1) / 2))


# the GPU comparison grid: n x outlier fraction, both cameras
GPU_GRID = [(seed, n, frac, cam)
            for seed, (n, cam) in enumerate([(30, "rand"), (100, "kitti"), (600, "kitti"), (2000, "rand"), (6000, "kitti")])
            for frac in (0.0, 0.3, 0.6)]
