"""so100_render on the MI355X: the HIP kernels against the host instantiation of the same header (tests/_rendercheck) and the
NumPy fp64 ray caster (tests/render_ref.py), env slicing and output bounds, no effect on the simulation, the 4096-env launch,
argument validation, the Gymnasium / SB3 render surface and `main.py record`'s video.

The device compiles with -ffp-contract=fast, the host instantiation with -ffp-contract=off: pixels on an edge may differ,
hence the same edge-tolerant bounds as tests/test_render_cpu.py."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import render_checks as T                                 # noqa: E402  (host instantiation + the pass conditions)
import render_ref as RR                                   # noqa: E402
from hostlibs import rendercheck                          # noqa: E402

SIZES = [(64, 64), (84, 84), (83, 61), (270, 480)]


@pytest.fixture(scope="module")
def H():
    return rendercheck()


@pytest.fixture(scope="module")
def stepped():
    """256 envs of Env01 under F_REFERENCE after 20 seeded random-action steps; qpos [N, 13] read back through get_state"""
    from so100_mujoco_rl_amd.lib import So100Sim, F_REFERENCE
    sim = So100Sim(1, 256, device="cuda:0", flags=F_REFERENCE, seed=3)
    sim.reset()
    g = torch.Generator(device="cuda:0"); g.manual_seed(7)
    for _ in range(20):
        sim.step(torch.rand(256, 6, device="cuda:0", generator=g) * 2 - 1)
    q, _ = sim.get_state()
    torch.cuda.synchronize()
    yield sim, q.t().contiguous().cpu().numpy().astype(np.float64)
    sim.close()


def _device_vs(host, dev, q, camera, W, Hh):
    """the pass conditions with the host instantiation as the reference image"""
    rgb_h, dep_h, seg_h = host
    rgb_d, dep_d, seg_d = dev
    eq = seg_d == seg_h
    if eq.mean() < 0.995:
        return f"segmentation equal on {eq.mean():.4f}"
    bad = ~eq & ~RR.near_edge(seg_h.astype(np.int64))
    if bad.any():
        return f"{int(bad.sum())} segmentation mismatches away from an edge"
    drel = np.abs(dep_d[eq].astype(np.float64) - dep_h[eq]) / dep_h[eq]
    if drel.max() > T.DEPTH_RTOL[camera]:
        return f"depth off by {drel.max():.2e}"
    par = RR.checker_parity(q, camera, W, Hh)
    ok = eq & ~RR.near_edge(np.where(seg_h == 1, par, -2))
    dr = np.abs(rgb_d.astype(np.int64) - rgb_h.astype(np.int64)).max(-1)[ok]
    if dr.size and dr.max() > 1:
        return f"rgb off by {dr.max()} LSB"
    return None


@pytest.mark.parametrize("camera", ["end", "scene"])
def test_hip_matches_host_and_numpy_reference(H, stepped, camera):
    sim, qpos = stepped
    cam = RR.CAM_END if camera == "end" else RR.CAM_SCENE
    fails = []
    checked = 0
    for W, Hh in SIZES:
        masks = [0, 1, 2, 4, 8, 15] if W == 64 else [0, 15]
        for mask in masks:
            out = sim.render(camera, W, Hh, geoms=mask, rgb=True, depth=True, segmentation=True)
            rgb, dep, seg = (out[k].cpu().numpy() for k in ("rgb", "depth", "segmentation"))
            envs = range(0, 256, 8) if W * Hh < 20000 else range(0, 256, 64)
            for e in envs:
                h = T.host_render(H, qpos[e], cam, W, Hh, mask)
                f = _device_vs((h[0][0], h[1][0], h[2][0]), (rgb[e], dep[e], seg[e]), qpos[e], cam, W, Hh)
                if f:
                    fails.append(("host", W, Hh, mask, e, f))
                checked += 1
            for e in (0, 97, 255):                        # and straight against the fp64 reference
                f = T.compare(rgb[e], dep[e], seg[e], qpos[e], cam, W, Hh, mask)
                if f:
                    fails.append(("numpy", W, Hh, mask, e, f))
    assert checked > 100 and not fails, fails[:5]


def test_env_slices_and_guard_bytes(stepped):
    sim, _ = stepped
    W, Hh, k, m = 83, 61, 37, 50
    full = sim.render("end", W, Hh, rgb=True, depth=True, segmentation=True)
    torch.cuda.synchronize()
    G = 64
    n_rgb, n_px = m * Hh * W * 3, m * Hh * W
    big_rgb = torch.full((n_rgb + 2 * G + 1,), 0xA5, dtype=torch.uint8, device="cuda:0")
    big_dep = torch.full((n_px + 2 * G,), -7.0, dtype=torch.float32, device="cuda:0")
    big_seg = torch.full((n_px + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda:0")
    out = {"rgb": big_rgb[G + 1:G + 1 + n_rgb].view(m, Hh, W, 3),          # odd byte offset: the byte-store path
           "depth": big_dep[G:G + n_px].view(m, Hh, W), "segmentation": big_seg[G:G + n_px].view(m, Hh, W)}
    part = sim.render("end", W, Hh, envs=slice(k, k + m), rgb=True, depth=True, segmentation=True, out=out)
    torch.cuda.synchronize()
    assert part["rgb"].data_ptr() == out["rgb"].data_ptr()
    for key in ("rgb", "depth", "segmentation"):
        assert torch.equal(part[key], full[key][k:k + m]), key
    assert bool((big_rgb[:G + 1] == 0xA5).all()) and bool((big_rgb[G + 1 + n_rgb:] == 0xA5).all())
    assert bool((big_dep[:G] == -7.0).all()) and bool((big_dep[G + n_px:] == -7.0).all())
    assert bool((big_seg[:G] == 0x5A).all()) and bool((big_seg[G + n_px:] == 0x5A).all())
    # (begin, count) and a 16-byte aligned frame size (the vector-store path) agree with the full render too
    f2 = sim.render("scene", 84, 84, segmentation=True, depth=True)
    p2 = sim.render("scene", 84, 84, envs=(k, m), segmentation=True, depth=True)
    for key in ("rgb", "depth", "segmentation"):
        assert torch.equal(p2[key], f2[key][k:k + m]), key


def test_render_does_not_perturb_the_simulation():
    from so100_mujoco_rl_amd.lib import So100Sim, F_REFERENCE
    sims = [So100Sim(3, 128, device="cuda:0", flags=F_REFERENCE, seed=9) for _ in range(2)]
    g = torch.Generator(device="cuda:0"); g.manual_seed(1)
    acts = [torch.rand(128, 6, device="cuda:0", generator=g) * 2 - 1 for _ in range(3)]
    for s in sims:
        s.reset()
        s.step(acts[0])
    before = [sims[0].get_field(n, dtype=torch.int32).clone() for n in sims[0].field_names()]
    sims[0].render("end", 64, 64, rgb=True, depth=True, segmentation=True)
    sims[0].render("scene", 64, 64, geoms=15)
    after = [sims[0].get_field(n, dtype=torch.int32) for n in sims[0].field_names()]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    for a in acts[1:]:
        r = [s.step(a) for s in sims]
        for x, y in zip(r[0], r[1]):
            assert torch.equal(x, y)
    for n in sims[0].field_names():
        assert torch.equal(sims[0].get_field(n, dtype=torch.int32), sims[1].get_field(n, dtype=torch.int32)), n
    for s in sims:
        s.close()


def test_4096_envs_one_launch(H):
    from so100_mujoco_rl_amd.lib import So100Sim, F_REFERENCE
    sim = So100Sim(3, 4096, device="cuda:0", flags=F_REFERENCE, seed=4)
    sim.reset()
    g = torch.Generator(device="cuda:0"); g.manual_seed(2)
    for _ in range(5):
        sim.step(torch.rand(4096, 6, device="cuda:0", generator=g) * 2 - 1)
    out = sim.render("end", 84, 84, rgb=True, depth=True, segmentation=True)
    q = sim.get_state()[0].t().contiguous().cpu().numpy().astype(np.float64)
    rgb, dep, seg = (out[k].cpu().numpy() for k in ("rgb", "depth", "segmentation"))
    assert rgb.shape == (4096, 84, 84, 3)
    rs = np.random.RandomState(0)
    fails = []
    for e in sorted(rs.choice(4096, 64, replace=False)):
        h = T.host_render(H, q[e], RR.CAM_END, 84, 84)
        f = _device_vs((h[0][0], h[1][0], h[2][0]), (rgb[e], dep[e], seg[e]), q[e], RR.CAM_END, 84, 84)
        if f:
            fails.append((e, f))
    assert not fails, fails[:5]
    assert len(np.unique(seg)) >= 2                       # the views are not all sky
    sim.close()


def test_invalid_render_io_is_rejected():
    from so100_mujoco_rl_amd import lib
    sim = lib.So100Sim(1, 16, device="cuda:0")
    L = lib.load()
    buf = torch.zeros(16 * 8 * 8 * 3, dtype=torch.uint8, device="cuda:0")
    fc = (C.c_float * 7)(0, 0, 0.1, 1.25, 45, -25, 45)

    def io(**kw):
        a = dict(camera=0, width=8, height=8, env_begin=0, env_count=16, geom_mask=0, free_cam=None, rgb_dev=buf.data_ptr(), depth_dev=None, seg_dev=None)
        a.update(kw)
        return lib.RenderIO(**a)

    good = io()
    assert L.so100_render(sim.h, C.byref(good), None) == 0
    cases = [(io(camera=2), b"camera"), (io(width=0), b"width"), (io(height=4097), b"height"), (io(width=4097), b"width"),
             (io(env_begin=-1), b"env_begin"), (io(env_begin=16), b"env_begin"), (io(env_begin=1), b"env_count"), (io(env_count=0), b"env_count"),
             (io(rgb_dev=None), b"NULL"), (io(free_cam=C.cast(fc, C.c_void_p)), b"free_cam"), (io(geom_mask=16), b"geom_mask")]
    for bad, word in cases:
        assert L.so100_render(sim.h, C.byref(bad), None) == -1
        assert word in L.so100_last_error(), (word, L.so100_last_error())
    assert L.so100_render(sim.h, C.byref(io(camera=1, free_cam=C.cast(fc, C.c_void_p))), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(lib.So100Error):
        sim.render("side")
    sim.close()


def test_gymnasium_and_vecenv_render():
    from so100_mujoco_rl_amd.envs import So100Env
    from so100_mujoco_rl_amd.vec_env import So100VecEnv
    assert So100Env.metadata["render_modes"] == ["rgb_array"]
    e = So100Env(1, render_mode="rgb_array"); e.reset()
    fr = e.render()
    assert isinstance(fr, np.ndarray) and fr.shape == (800, 800, 3) and fr.dtype == np.uint8
    e.close()
    e = So100Env(3, render_mode="rgb_array"); e.reset()
    e.step(np.zeros(6, np.float32))
    fr = e.render()
    wrist = e.sim.render("end", 270, 480, envs=(0, 1))["rgb"][0].flip(0).cpu().numpy()
    assert fr.shape == (800, 800, 3) and np.array_equal(fr[-480:, :270], wrist)
    scene = e.sim.render("scene", envs=(0, 1))["rgb"][0].cpu().numpy()
    assert np.array_equal(fr[:-480], scene[:-480]) and np.array_equal(fr[-480:, 270:], scene[-480:, 270:])
    e.close()
    e = So100Env(1); e.reset()
    assert e.render() is None
    e.close()
    v = So100VecEnv("Env01-v1", 16, render_mode="rgb_array", render_envs=4)
    v.reset()
    ims = v.get_images()
    assert isinstance(ims, list) and len(ims) == 16 and all(im.shape == (800, 800, 3) for im in ims[:4]) and all(im is None for im in ims[4:])
    big = v.render()
    assert big.shape == (1600, 1600, 3) and np.array_equal(big[:800, 800:], ims[1]) and np.array_equal(big[800:, :800], ims[2])
    v.close()
    v = So100VecEnv("Env01-v1", 4)
    assert v.render() is None and v.get_images() == [None] * 4
    v.close()


def test_record_writes_a_video(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from PIL import Image
    from so100_mujoco_rl_amd import main as drv
    from so100_mujoco_rl_amd.ppo import ActorCritic
    monkeypatch.chdir(tmp_path)
    model = tmp_path / "untrained.pt"
    torch.save(ActorCritic(8).state_dict(), model)                 # the package's native checkpoint format (main.py _load_native)
    r = CliRunner().invoke(drv.cli, ["-a", "PPO", "-m", str(model), "record", "-e", "Env03-v1", "--steps", "64"], catch_exceptions=False)
    assert r.exit_code == 0
    traj = np.load(tmp_path / "movies" / "Env03-v1_PPO.npz")["trajectory"]
    assert traj.shape == (64, 13 + 12 + 8 + 6)
    chunks, frames, idx, _, _ = T.parse_avi(str(tmp_path / "movies" / "rec-Env03-v1-step-0-to-step-64.avi"))
    assert struct.unpack("<10I", chunks[b"avih"][:40])[4] == 64 and len(frames) == 64 and len(idx) == 64
    for jpg in frames[::9]:
        im = np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))
        assert im.shape == (800, 800, 3) and im.std() > 5
