"""NumPy fp64 ray caster of the render model (DESIGN.md "Rendering"), written from the model's description alone: it shares
no code with csrc/so100_render.hpp.  Every pose comes from the CPU oracle: set Data.qpos, call so100o_kinematics, read
cam_xpos / cam_xmat, xpos / xmat and the model's prox_* / pad_* geometry.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from oracle import so100_oracle as O

CAM_END, CAM_SCENE = 0, 1
G_FLOOR, G_CUBE, G_LINKS, G_PADS = 1, 2, 4, 8
DEFAULT_MASK = {CAM_END: G_FLOOR | G_CUBE, CAM_SCENE: G_FLOOR | G_CUBE | G_LINKS}
DEFAULT_SIZE = {CAM_END: (1080, 1920), CAM_SCENE: (800, 800)}        # (W, H)
FOVY = {CAM_END: 120.0, CAM_SCENE: 45.0}
SCENE_CAM = dict(lookat=(0.0, 0.0, 0.1), distance=1.25, azimuth=45.0, elevation=-25.0)
ZNEAR, ZFAR = 0.01 * 0.8, 50.0 * 0.8
CUBE_BODY, CUBE_HALF = 8, 0.01
AMBIENT, HEAD, LIGHT = 0.3, 0.6, 0.7
L_DIR = np.array([0.5, 0.5, 1.0]) / np.linalg.norm([0.5, 0.5, 1.0])
CHECK_A, CHECK_B = np.array([0.2, 0.3, 0.4]), np.array([0.1, 0.2, 0.3])
RGB_CUBE, RGB_LINK, RGB_PAD = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.331, 0.0]), np.array([0.5, 0.5, 0.5])


def free_camera(lookat, distance, azimuth, elevation):
    """MuJoCo free camera: (position, R) with the columns of R the camera's x (right), y (up), z (-forward) axes."""
    a, e = np.radians(azimuth), np.radians(elevation)
    fwd = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    up = np.array([-np.sin(e) * np.cos(a), -np.sin(e) * np.sin(a), np.cos(e)])
    return np.asarray(lookat, float) - distance * fwd, np.stack([np.cross(fwd, up), up, -fwd], axis=1)


def kinematics(qpos):
    d = O.Data()
    for i in range(13):
        d.qpos[i] = float(qpos[i])
    O.lib().so100o_kinematics(C.byref(O.model()), C.byref(d))
    return d


def camera_rays(camera, W, H, fovy):
    """camera-frame directions (x, y, -1) of every pixel, [H, W, 3]"""
    f = 0.5 * H / np.tan(np.radians(fovy) / 2)
    c = (np.arange(W) + 0.5 - W / 2) / f
    r = np.arange(H) + 0.5
    y = (r - H / 2) / f if camera == CAM_END else (H / 2 - r) / f
    X, Y = np.meshgrid(c, y)
    return np.stack([X, Y, -np.ones_like(X)], axis=-1)


def _box(o, dn, cen, R, h):
    """entry t and normal of a box (centre, rotation with the box axes as columns, half sizes); t = inf where missed"""
    ob = (o - cen) @ R                      # [3]
    db = dn @ R                             # [..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-h - ob) / db
        t2 = (h - ob) / db
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    ax = np.argmax(lo, axis=-1)
    tn = np.take_along_axis(lo, ax[..., None], -1)[..., 0]
    tf = hi.min(axis=-1)
    hit = tn <= tf
    sgn = -np.sign(np.take_along_axis(db, ax[..., None], -1)[..., 0])
    n = sgn[..., None] * R.T[ax]
    return np.where(hit, tn, np.inf), n


def _sphere(o, dn, c, r):
    oc = o - c
    b = dn @ oc
    disc = b * b - (oc @ oc - r * r)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where(disc >= 0, t, np.inf)


def _capsule(o, dn, a, b, r):
    ax = b - a
    ln = np.linalg.norm(ax)
    u = ax / ln
    oc = o - a
    du, ou = dn @ u, oc @ u
    dp = dn - du[..., None] * u
    op = oc - ou * u
    A = (dp * dp).sum(-1)
    B = dp @ op
    Cc = op @ op - r * r
    disc = B * B - A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        tcyl = (-B - np.sqrt(disc)) / A
    y = ou + tcyl * du
    tcyl = np.where((disc >= 0) & (A > 1e-12) & (y >= 0) & (y <= ln), tcyl, np.inf)
    ta, tb = _sphere(o, dn, a, r), _sphere(o, dn, b, r)
    t = np.minimum(tcyl, np.minimum(ta, tb))
    p = oc + np.where(np.isfinite(t), t, 0.0)[..., None] * dn
    yy = np.where(tcyl <= np.minimum(ta, tb), (p @ u), np.where(ta <= tb, 0.0, ln))
    n = (p - yy[..., None] * u) / r
    return t, n


def render(qpos, camera, W=None, H=None, mask=0, free_cam=None):
    """(rgb uint8 [H, W, 3], depth float64 [H, W], seg uint8 [H, W]) of one env state qpos[13].
    free_cam: (lookat x, y, z, distance, azimuth, elevation, fovy) for the scene camera."""
    W0, H0 = DEFAULT_SIZE[camera]
    W, H = W or W0, H or H0
    mask = mask or DEFAULT_MASK[camera]
    m, d = O.model(), kinematics(qpos)
    if camera == CAM_END:
        o, R, fovy = np.array(d.cam_xpos), np.array(d.cam_xmat).reshape(3, 3), FOVY[CAM_END]
    else:
        fc = list(SCENE_CAM["lookat"]) + [SCENE_CAM["distance"], SCENE_CAM["azimuth"], SCENE_CAM["elevation"], FOVY[CAM_SCENE]] \
            if free_cam is None else [float(v) for v in free_cam]
        o, R = free_camera(fc[:3], fc[3], fc[4], fc[5])
        fovy = fc[6]
    dc = camera_rays(camera, W, H, fovy)
    dw = dc @ R.T
    dl = np.linalg.norm(dw, axis=-1)
    dn = dw / dl[..., None]
    best = np.full((H, W), ZFAR)             # camera-axis depth
    seg = np.zeros((H, W), np.uint8)
    nrm = np.zeros((H, W, 3))
    base = np.zeros((H, W, 3))

    def take(t, n, gid, col):
        s = t / dl
        upd = np.isfinite(s) & (s >= ZNEAR) & (s < best)
        best[upd] = s[upd]
        seg[upd] = gid
        nrm[upd] = n[upd] if n.ndim == 3 else n
        base[upd] = col[upd] if col.ndim == 3 else col

    xpos, xmat = np.array(d.xpos), np.array(d.xmat).reshape(-1, 3, 3)
    if mask & G_FLOOR:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(dn[..., 2] < 0, -o[2] / dn[..., 2], np.inf)
        t = np.where(t > 0, t, np.inf)
        p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * dn
        even = ((np.floor(p[..., 0] / 0.1) + np.floor(p[..., 1] / 0.1)) % 2) == 0
        take(t, np.array([0.0, 0.0, 1.0]), 1, np.where(even[..., None], CHECK_A, CHECK_B))
    if mask & G_CUBE:
        t, n = _box(o, dn, xpos[CUBE_BODY], xmat[CUBE_BODY], np.full(3, CUBE_HALF))
        take(t, n, 2, RGB_CUBE)
    if mask & G_LINKS:
        pp = np.array(m.prox_p).reshape(5, 2, 3)
        for k in range(5):
            b = m.prox_body[k]
            a_w, b_w = xpos[b] + xmat[b] @ pp[k, 0], xpos[b] + xmat[b] @ pp[k, 1]
            t, n = _capsule(o, dn, a_w, b_w, m.prox_radius[k])
            take(t, n, 3 + k, RGB_LINK)
    if mask & G_PADS:
        ppos, psz = np.array(m.pad_pos).reshape(8, 3), np.array(m.pad_size).reshape(8, 3)
        for g in range(8):
            b = m.pad_body[g]
            t, n = _box(o, dn, xpos[b] + xmat[b] @ ppos[g], xmat[b], psz[g])
            take(t, n, 8 + g, RGB_PAD)
    k = AMBIENT + HEAD * np.maximum(0.0, nrm @ R[:, 2]) + LIGHT * np.maximum(0.0, nrm @ L_DIR)
    c = base * k[..., None]
    sky = 0.8 * 0.5 * (1.0 + dn[..., 2])
    c = np.where((seg == 0)[..., None], sky[..., None], c)
    rgb = np.floor(255.0 * np.clip(c, 0.0, 1.0) + 0.5).astype(np.uint8)
    return rgb, best, seg


def checker_parity(qpos, camera, W=None, H=None, free_cam=None):
    """floor-checker parity of every pixel's floor point (-1 where the ray does not reach the floor): where a square's edge runs"""
    W0, H0 = DEFAULT_SIZE[camera]
    W, H = W or W0, H or H0
    d = kinematics(qpos)
    if camera == CAM_END:
        o, R, fovy = np.array(d.cam_xpos), np.array(d.cam_xmat).reshape(3, 3), FOVY[CAM_END]
    else:
        fc = list(SCENE_CAM["lookat"]) + [SCENE_CAM["distance"], SCENE_CAM["azimuth"], SCENE_CAM["elevation"], FOVY[CAM_SCENE]] \
            if free_cam is None else [float(v) for v in free_cam]
        o, R = free_camera(fc[:3], fc[3], fc[4], fc[5])
        fovy = fc[6]
    dn = camera_rays(camera, W, H, fovy) @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[2] / dn[..., 2]
    p = o + np.where(t > 0, t, 0.0)[..., None] * dn
    par = ((np.floor(p[..., 0] / 0.1) + np.floor(p[..., 1] / 0.1)) % 2).astype(np.int64)
    return np.where(t > 0, par, -1)


def near_edge(label):
    """True where a pixel or one of its 8 neighbours carries a different label"""
    H, W = label.shape
    pad = np.pad(label, 1, mode="edge")
    out = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != label
    return out
