"""Many cameras of one scene, three routes, wall-clock per batch (one GPU call):

    (a) Scene(...) + render per view          re-upload: SBVH build, tables, textures for every camera
    (b) set_camera + render per view          one upload, one render call per camera
    (c) one render_views                      one upload, one pass over all cameras

Scenes cbox and disney_bsdf, 64 cameras on a circle around the bounds centre, films 64 x 64 and 256 x 256 at 16 spp.  After a warm-up of
each shape the three routes alternate, 5 rounds; medians and the spread (min .. max) are reported.  Host wall-clock around the calls, so
everything a caller pays is inside: upload, pixel lists, launches, the copy of the frames to the host.

    python tools/views_time.py [--out profiles/views_time.txt] [--views 64] [--rounds 5]
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import lajolla_public_amd as lj  # noqa: E402
from lajolla_public_amd import _abi  # noqa: E402

SCENES = {"cbox": os.path.join(ROOT, "scenes", "cbox", "cbox.xml"),
          "disney_bsdf": os.path.join(ROOT, "scenes", "disney_bsdf_test", "disney_bsdf.xml")}


def circle_cameras(hs, info, n, width, height):
    """n cameras on a circle around the bounds centre, in the plane normal to the parsed camera's up vector, at the parsed camera's
    distance and fov, looking at the centre."""
    c = hs.desc.camera
    m = np.array(list(c.cam_to_world)).reshape(4, 4)
    org, up = m[:3, 3], m[:3, 1] / np.linalg.norm(m[:3, 1])
    centre = np.array(list(info.bounds_center))
    fov = math.degrees(2.0 * math.atan(1.0 / (-2.0 * c.cam_to_sample[0])))
    arm = org - centre
    arm = arm - up * arm.dot(up)
    radius, lift = np.linalg.norm(arm), (org - centre).dot(up)
    a0, a1 = arm / radius, np.cross(up, arm / radius)
    cams = []
    for i in range(n):
        t = 2.0 * math.pi * i / n
        o = centre + up * lift + radius * (math.cos(t) * a0 + math.sin(t) * a1)
        cams.append(lj.look_at_camera(o, centre, up, fov, width, height, c.filter_kind, c.filter_param, c.medium_id))
    return cams


def with_camera(path, cam):
    hs = lj.parse_scene(path)
    C.memmove(C.addressof(hs.desc.camera), C.addressof(cam), C.sizeof(_abi.LjCamera))
    return hs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    ctx = lj.Context(0)
    lines = [f"{args.views} views, {args.spp} spp, {args.rounds} alternating rounds per route after one warm-up; wall-clock ms per batch: median (min .. max)",
             "(a) Scene + render per view   (b) set_camera + render per view   (c) one render_views",
             f"{'scene':12s} {'film':9s} {'(a) re-upload':>26s} {'(b) set_camera':>26s} {'(c) render_views':>26s}   c/b    (c) Msamples/s"]
    for name, path in SCENES.items():
        hs0 = lj.parse_scene(path)
        info = lj.Scene(ctx, hs0).info
        for w, h in ((64, 64), (256, 256)):
            cams = circle_cameras(hs0, info, args.views, w, h)
            host_scenes = [with_camera(path, cam) for cam in cams]   # parsed outside the timed region: route (a) is charged the upload only
            sc = lj.Scene(ctx, host_scenes[0])

            def route_a():
                return [lj.render(lj.Scene(ctx, hs), spp=args.spp) for hs in host_scenes]

            def route_b():
                out = []
                for cam in cams:
                    sc.set_camera(cam)
                    out.append(lj.render(sc, spp=args.spp))
                return out

            def route_c():
                return lj.render_views(sc, cams, spp=args.spp)

            routes = (route_a, route_b, route_c)
            first = [np.stack(r()) if r is not route_c else r() for r in routes]   # warm-up; the three routes must agree bit for bit
            assert all(np.array_equal(first[0], f) for f in first[1:]), "the three routes disagree"
            times = [[], [], []]
            for _ in range(args.rounds):
                for i, r in enumerate(routes):
                    t0 = time.perf_counter()
                    r()
                    times[i].append(1e3 * (time.perf_counter() - t0))
            med = [statistics.median(t) for t in times]
            cell = lambda t: f"{statistics.median(t):9.2f} ({min(t):7.2f} .. {max(t):7.2f})"
            rate = args.views * w * h * args.spp / (med[2] * 1e-3) / 1e6
            lines.append(f"{name:12s} {w:4d}x{h:<4d} {cell(times[0]):>26s} {cell(times[1]):>26s} {cell(times[2]):>26s}  {med[2] / med[1]:5.2f}  {rate:10.1f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
