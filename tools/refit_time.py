"""A moved scene, two routes, wall-clock per frame (one GPU call):

    (a) Scene(ctx, moved)                     re-upload: SBVH build, mip pyramids, environment-map and light tables
    (b) scene.update_geometry(moved)          re-derive what depends on positions, refit the BVHs on the device; host and device part
    (c) render at the parsed pose on the refitted tree against the freshly built one, every vertex displaced by 0, 1 % and 10 % of the bounds radius

Scenes cbox, disney_bsdf and sponza.  After one warm-up the routes alternate, 5 rounds; medians and the spread (min .. max) are reported.
(a) and (b) are host wall-clock around the calls; the device part of (b) is the time between two events around its copies and launches
(LjStats.render_ms), the host part the re-derivation (LjStats.generate_ms).  (c) is LjStats.render_ms of one render; the two images must be
bit-identical.

    python tools/refit_time.py [--out profiles/refit_time.txt] [--rounds 5] [--spp 16]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import lajolla_public_amd as lj  # noqa: E402

SCENES = {"cbox": os.path.join(ROOT, "scenes", "cbox", "cbox.xml"),
          "disney_bsdf": os.path.join(ROOT, "scenes", "disney_bsdf_test", "disney_bsdf.xml"),
          "sponza": os.path.join(ROOT, "scenes", "sponza", "sponza.xml")}


def displace(hs, P0, R, amplitude):
    P = hs.positions_view()
    P[:] = P0 + amplitude * R * np.sin((9.0 / R) * P0[:, [1, 2, 0]] + np.array([0.3, 1.1, 2.0]))


def cell(t):
    return f"{statistics.median(t):9.2f} ({min(t):8.2f} .. {max(t):8.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    ctx = lj.Context(0)
    lines = [f"every vertex displaced by a R sin(k p), R = bounds radius; {args.rounds} alternating rounds after one warm-up; ms: median (min .. max)",
             "(a) Scene(ctx, moved): wall-clock   (b) update_geometry(moved): wall-clock = host re-derivation + device (table copies, refit launches) + readback",
             f"(c) one render of the full film at {args.spp} spp, device time: on the refitted tree | on the freshly built tree; images asserted bit-identical"]
    for name, path in SCENES.items():
        hs = lj.parse_scene(path)
        P0 = hs.positions()
        sc = lj.Scene(ctx, hs)
        R = sc.info.bounds_radius
        lines.append(f"{name}: {sc.info.n_triangles} triangles, {sc.info.n_spheres} spheres, {sc.info.n_bvh_nodes} BVH4 nodes, film {sc.info.width} x {sc.info.height}")
        for amp in (0.0, 0.01, 0.1):
            displace(hs, P0, R, amp)
            t_up, t_upd, t_host, t_dev, t_refit, t_fresh = [], [], [], [], [], []
            for rnd in range(args.rounds + 1):
                t0 = time.perf_counter()
                fresh = lj.Scene(ctx, hs)
                ta = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                sc.update_geometry(hs)
                tb = 1e3 * (time.perf_counter() - t0)
                st = sc.stats()
                host_ms, dev_ms = st.generate_ms, st.render_ms
                img_r = lj.render(sc, spp=args.spp)
                r_ms = sc.stats().render_ms
                img_f = lj.render(fresh, spp=args.spp)
                f_ms = fresh.stats().render_ms
                assert np.array_equal(img_r.view(np.uint32), img_f.view(np.uint32)), f"{name} amplitude {amp}: refitted and fresh images differ"
                del fresh
                if rnd == 0:
                    continue   # warm-up
                t_up.append(ta); t_upd.append(tb); t_host.append(host_ms); t_dev.append(dev_ms); t_refit.append(r_ms); t_fresh.append(f_ms)
            lines.append(f"  amplitude {amp:4.2f} R  (a) upload {cell(t_up)}   (b) update {cell(t_upd)} = host {cell(t_host)} + device {cell(t_dev)}")
            lines.append(f"                    (c) render refitted {cell(t_refit)} | fresh {cell(t_fresh)}   refitted / fresh {statistics.median(t_refit) / statistics.median(t_fresh):5.3f}"
                         f"   upload / update {statistics.median(t_up) / statistics.median(t_upd):6.1f}")
            print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
