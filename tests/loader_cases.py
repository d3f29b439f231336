"""The random sensor folder that the loader tests share (test infrastructure, no tests in here)."""
import numpy as np
from PIL import Image
from scipy.spatial.transform import Rotation


def make_sensor_folder(folder, n, rng, cw=64, ch=48, dw=32, dh=24):
    """n random colour / depth / pose frames and the two intrinsics files in the reference's layout; returns (Kc, Kd, [(colour, depth, pose)])"""
    folder.mkdir()
    Kc = np.eye(4); Kc[0, 0] = 70.0; Kc[1, 1] = 71.0; Kc[0, 2] = 31.5; Kc[1, 2] = 23.5
    Kd = np.eye(4); Kd[0, 0] = 35.0; Kd[1, 1] = 35.5; Kd[0, 2] = 15.5; Kd[1, 2] = 11.5
    np.savetxt(folder / "colorIntrinsics.txt", Kc); np.savetxt(folder / "depthIntrinsics.txt", Kd)
    data = []
    for i in range(n):
        col = rng.integers(0, 256, (ch, cw, 3), np.uint8)
        dep = rng.integers(0, 3000, (dh, dw)).astype(np.uint16)
        T = np.eye(4); T[:3, :3] = Rotation.from_rotvec(rng.normal(size=3) * 0.3).as_matrix(); T[:3, 3] = rng.normal(size=3)
        Image.fromarray(col).save(folder / f"frame-{i:06d}.color.png")
        Image.fromarray(dep).save(folder / f"frame-{i:06d}.depth.png")
        np.savetxt(folder / f"frame-{i:06d}.pose.txt", T)
        data.append((col, dep, T))
    return Kc, Kd, data
