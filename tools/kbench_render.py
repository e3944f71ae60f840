"""Time so100_render (scene kernel + pixel kernel, one so100_render call) with HIP events after warm-up; one JSON line per case.

    python tools/kbench_render.py [--iters 50] [--warmup 10]

Cases: 4096 envs x 84 x 84 end RGB; 4096 x 128 x 128 end RGB + depth + segmentation; 1 x 1080 x 1920 end; 1 x 800 x 800 scene with
every geometry bit.  Each line: us per call, frames/s, bytes written and their share of HBM bandwidth (6.29 TB/s measured),
rays/s.  The envs are Env03 under F_REFERENCE after a few random steps (arms and cubes spread over their start region)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from so100_mujoco_rl_amd.lib import So100Sim, F_REFERENCE  # noqa: E402

HBM_BPS = 6.29e12
CASES = [
    dict(name="end_4096x84x84_rgb", n=4096, camera="end", W=84, H=84, rgb=True, depth=False, seg=False, geoms=None),
    dict(name="end_4096x128x128_rgb_depth_seg", n=4096, camera="end", W=128, H=128, rgb=True, depth=True, seg=True, geoms=None),
    dict(name="end_1x1080x1920_rgb", n=1, camera="end", W=1080, H=1920, rgb=True, depth=False, seg=False, geoms=None),
    dict(name="scene_1x800x800_rgb_all_geoms", n=1, camera="scene", W=800, H=800, rgb=True, depth=False, seg=False, geoms=15),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None, help="run only the case with this name")
    a = ap.parse_args()
    sims = {}
    for c in CASES:
        if a.only and c["name"] != a.only:
            continue
        sim = sims.get(c["n"])
        if sim is None:
            sim = sims[c["n"]] = So100Sim(3, c["n"], device="cuda:0", flags=F_REFERENCE, seed=1)
            sim.reset()
            g = torch.Generator(device="cuda:0"); g.manual_seed(0)
            for _ in range(8):
                sim.step(torch.rand(c["n"], 6, device="cuda:0", generator=g) * 2 - 1)
        kw = dict(camera=c["camera"], width=c["W"], height=c["H"], geoms=c["geoms"], rgb=c["rgb"], depth=c["depth"], segmentation=c["seg"])
        out = sim.render(**kw)
        for _ in range(a.warmup):
            sim.render(out=out, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            sim.render(out=out, **kw)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        px = c["n"] * c["W"] * c["H"]
        nbytes = px * (3 * c["rgb"] + 4 * c["depth"] + 1 * c["seg"])
        print(json.dumps({"case": c["name"], "envs": c["n"], "width": c["W"], "height": c["H"], "camera": c["camera"],
                          "us_per_call": round(us, 2), "frames_per_s": round(c["n"] / (us * 1e-6), 1), "bytes_written": nbytes,
                          "hbm_share": round(nbytes / (us * 1e-6) / HBM_BPS, 4), "rays_per_s": round(px / (us * 1e-6), 1),
                          "iters": a.iters, "device": torch.cuda.get_device_name(0)}), flush=True)
    for s in sims.values():
        s.close()


if __name__ == "__main__":
    main()
