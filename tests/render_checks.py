"""What the CPU and the GPU render tests share: the host instantiation's render call, the pass conditions against the NumPy fp64 ray
caster (tests/render_ref.py) and a reader for the Motion-JPEG AVI files that MjpegAviWriter and `main.py record` write."""
import struct

import numpy as np

import render_ref as RR

# depth bound: the scene camera's pose is exact, the wrist camera's comes from fp32 FK (task_poses: 1e-7 m / 2e-7 rad off the
# oracle), which grazing floor rays and 3 cm-near pads turn into up to 5e-5 relative depth (DESIGN.md "Rendering")
DEPTH_RTOL = {RR.CAM_END: 1e-4, RR.CAM_SCENE: 1e-5}


def host_render(H, qpos, camera, W, Hh, mask=0, free_cam=None):
    """host instantiation: (rgb [n, H, W, 3], depth [n, H, W], seg [n, H, W]) of qpos [n, 13]"""
    q = np.ascontiguousarray(np.asarray(qpos, np.float32).reshape(-1, 13))
    n = q.shape[0]
    rgb = np.zeros((n, Hh, W, 3), np.uint8); dep = np.zeros((n, Hh, W), np.float32); seg = np.zeros((n, Hh, W), np.uint8)
    fc = None if free_cam is None else np.ascontiguousarray(free_cam, np.float32)
    H.rc_render(q.ctypes.data, n, camera, W, Hh, mask, None if fc is None else fc.ctypes.data, rgb.ctypes.data, dep.ctypes.data, seg.ctypes.data, None)
    return rgb, dep, seg


def compare(rgb, dep, seg, q, camera, W, Hh, mask, free_cam=None):
    """the pass conditions against render_ref; returns a short failure string or None"""
    r2, d2, s2 = RR.render(q, camera, W, Hh, mask, free_cam)
    eq = seg == s2
    if eq.mean() < 0.995:
        return f"segmentation equal on {eq.mean():.4f} of the pixels"
    bad = ~eq & ~RR.near_edge(s2.astype(np.int64))
    if bad.any():
        return f"{int(bad.sum())} segmentation mismatches away from an edge"
    drel = np.abs(dep[eq].astype(np.float64) - d2[eq]) / d2[eq]
    if drel.max() > DEPTH_RTOL[camera]:
        return f"depth off by {drel.max():.2e} relative"
    # a checker square's edge is an edge of the image too (floor pixels whose 8-neighbourhood spans two squares)
    par = RR.checker_parity(q, camera, W, Hh, free_cam)
    ok = eq & ~RR.near_edge(np.where(s2 == 1, par, -2))
    dr = np.abs(rgb.astype(np.int64) - r2.astype(np.int64)).max(-1)[ok]
    if dr.size and dr.max() > 1:
        return f"rgb off by {dr.max()} LSB"
    return None


def parse_avi(path):
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    chunks = {}
    frames = []
    idx = []
    movi = None

    def walk(lo, hi):
        nonlocal movi
        p = lo
        while p < hi:
            cid, size = struct.unpack("<4sI", data[p:p + 8])
            if cid == b"LIST":
                kind = data[p + 8:p + 12]
                if kind == b"movi":
                    movi = p + 8
                walk(p + 12, p + 8 + size)
            elif cid == b"00dc":
                frames.append(data[p + 8:p + 8 + size])
            elif cid == b"idx1":
                for k in range(size // 16):
                    idx.append(struct.unpack("<4sIII", data[p + 8 + 16 * k:p + 24 + 16 * k]))
            else:
                chunks[cid] = data[p + 8:p + 8 + size]
            p += 8 + size + (size & 1)
    walk(12, len(data))
    return chunks, frames, idx, movi, data
