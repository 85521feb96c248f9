"""A moved scene, three trees, wall-clock per frame (one GPU call) — tools/refit_time.py with the rebuild beside the refit:

    (a) Scene(ctx, moved)                          re-upload: SBVH build, mip pyramids, environment-map and light tables
    (b) scene.update_geometry(moved)               re-derive what depends on positions, refit the BVHs on the device
    (r) scene.update_geometry(moved, rebuild=True) the same, then lj_scene_rebuild_bvh: a linear BVH built on the device, collapsed on the host, refitted
    (c) render on the refitted tree, on the rebuilt tree and on the freshly built one, every vertex displaced by 0, 1 % and 10 % of the bounds radius

Scenes cbox (a leaf-scan scene: the rebuild is a no-op), disney_bsdf and sponza.  Two scenes are kept beside the fresh one: `ref` is only ever
updated (the upload's SBVH topology, refitted), `reb` is updated and rebuilt.  After one warm-up the routes alternate, 5 rounds; medians
and the spread (min .. max) are reported.  (a), (b) and (r) are host wall-clock around the calls; the parts of the rebuild are
LjRebuildStats (build: the device's linear BVH and its readback; emit: the host's collapse and level tables; refit: upload of the trees and
the refit launches).  (c) is LjStats.render_ms of one render; the three images must be bit-identical.

--builder names further builders to measure beside the linear one, in the same alternating rounds: "ploc" or "ploc:RADIUS", comma-separated
(lj_scene_rebuild_bvh_ex).  Each gets a scene of its own that is updated and rebuilt with it, one more line of rebuild times with the rounds
of clustering (LjBuildStats), and one more line of frame times against the linear builder's tree and the fresh one.  The default, "lbvh",
adds nothing: the output is the one described above.  --append adds to --out instead of replacing it.

    python tools/rebuild_time.py [--out profiles/rebuild_time.txt] [--append] [--rounds 5] [--spp 16] [--scenes cbox,disney_bsdf,sponza] [--builder lbvh,ploc:8,ploc:16]
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
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--builder", default="lbvh")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    extra = []   # (label, builder, radius) of every builder beside the linear one
    for b in args.builder.split(","):
        kind, _, radius = b.partition(":")
        if kind != "lbvh":
            extra.append((b, kind, int(radius) if radius else None))
    ctx = lj.Context(0)
    lines = [f"every vertex displaced by a R sin(k p), R = bounds radius; {args.rounds} alternating rounds after one warm-up; ms: median (min .. max)",
             "(a) Scene(ctx, moved): wall-clock   (b) update_geometry(moved): wall-clock   (r) update_geometry(moved, rebuild=True): wall-clock; the rebuild's parts:",
             "    build = the device's linear BVH + readback, emit = host collapse into BVH4 / BVH8 + level tables, refit = upload of the trees + refit launches",
             f"(c) one render of the full film at {args.spp} spp, device time: on the refitted tree | on the rebuilt tree | on the freshly built tree; images asserted bit-identical"]
    if extra:
        lines.append("further builders (" + ", ".join(e[0] for e in extra) + "): update_geometry + rebuild_bvh(builder, radius), wall-clock, its parts as above, cluster = the rounds of "
                     "clustering within build; the frame on its tree against the linear builder's and the fresh one")
    for name in args.scenes.split(","):
        hs = lj.parse_scene(SCENES[name])
        P0 = hs.positions()
        ref, reb = lj.Scene(ctx, hs), lj.Scene(ctx, hs)
        others = [lj.Scene(ctx, hs) for _ in extra]
        R = ref.info.bounds_radius
        lines.append(f"{name}: {ref.info.n_triangles} triangles, {ref.info.n_spheres} spheres, {ref.info.n_bvh_nodes} BVH4 nodes, film {ref.info.width} x {ref.info.height}")
        for amp in (0.0, 0.01, 0.1):
            displace(hs, P0, R, amp)
            t = {k: [] for k in ("up", "upd", "reb", "build", "emit", "refit", "r_ref", "r_reb", "r_fresh")}
            tx = [{k: [] for k in ("reb", "build", "cluster", "emit", "refit", "render")} for _ in extra]
            for rnd in range(args.rounds + 1):
                t0 = time.perf_counter()
                fresh = lj.Scene(ctx, hs)
                ta = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                ref.update_geometry(hs)
                tb = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                reb.update_geometry(hs, rebuild=True)
                tr = 1e3 * (time.perf_counter() - t0)
                rs = lj.rebuild_stats(reb)
                img_ref = lj.render(ref, spp=args.spp)
                ref_ms = ref.stats().render_ms
                img_reb = lj.render(reb, spp=args.spp)
                reb_ms = reb.stats().render_ms
                img_f = lj.render(fresh, spp=args.spp)
                f_ms = fresh.stats().render_ms
                assert np.array_equal(img_ref.view(np.uint32), img_f.view(np.uint32)), f"{name} amplitude {amp}: refitted and fresh images differ"
                assert np.array_equal(img_reb.view(np.uint32), img_f.view(np.uint32)), f"{name} amplitude {amp}: rebuilt and fresh images differ"
                got = []
                for (label, kind, radius), sc in zip(extra, others):
                    t0 = time.perf_counter()
                    sc.update_geometry(hs)
                    sc.rebuild_bvh(builder=kind, radius=radius)
                    tx_reb = 1e3 * (time.perf_counter() - t0)
                    xs, xb = lj.rebuild_stats(sc), lj.build_stats(sc)
                    img = lj.render(sc, spp=args.spp)
                    assert np.array_equal(img.view(np.uint32), img_f.view(np.uint32)), f"{name} amplitude {amp}: {label} and fresh images differ"
                    got.append((dict(reb=tx_reb, build=xs.build_ms, cluster=xb.cluster_ms, emit=xs.emit_ms, refit=xs.refit_ms, render=sc.stats().render_ms), xs, xb))
                del fresh
                if rnd == 0:
                    continue   # warm-up
                for acc, (vals, _, _) in zip(tx, got):
                    for k, v in vals.items():
                        acc[k].append(v)
                for k, v in (("up", ta), ("upd", tb), ("reb", tr), ("build", rs.build_ms), ("emit", rs.emit_ms), ("refit", rs.refit_ms), ("r_ref", ref_ms), ("r_reb", reb_ms), ("r_fresh", f_ms)):
                    t[k].append(v)
            m = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"  amplitude {amp:4.2f} R  (a) upload {cell(t['up'])}   (b) update {cell(t['upd'])}   (r) update + rebuild {cell(t['reb'])}")
            lines.append(f"                    rebuilt {rs.rebuilt}: build {cell(t['build'])} + emit {cell(t['emit'])} + refit {cell(t['refit'])}; {rs.n_nodes4} BVH4 nodes depth {rs.depth4}, {rs.n_nodes8} BVH8 nodes depth {rs.depth8}, {rs.n_leaves} leaves")
            lines.append(f"                    (c) render refitted {cell(t['r_ref'])} | rebuilt {cell(t['r_reb'])} | fresh {cell(t['r_fresh'])}"
                         f"   refitted / fresh {m['r_ref'] / m['r_fresh']:5.3f}   rebuilt / fresh {m['r_reb'] / m['r_fresh']:5.3f}   rebuilt / refitted {m['r_reb'] / m['r_ref']:5.3f}")
            for (label, _, _), acc, (_, xs, xb) in zip(extra, tx, got):
                mr = statistics.median(acc["render"])
                lines.append(f"                    {label}: update + rebuild {cell(acc['reb'])}: build {cell(acc['build'])} (cluster {cell(acc['cluster'])}, {xb.rounds} rounds, {xb.tail_rounds} in the tail) "
                             f"+ emit {cell(acc['emit'])} + refit {cell(acc['refit'])}; {xs.n_nodes4} BVH4 nodes depth {xs.depth4}, {xs.n_nodes8} BVH8 nodes depth {xs.depth8}, {xs.n_leaves} leaves")
                lines.append(f"                    {label}: (c) render {cell(acc['render'])}   / fresh {mr / m['r_fresh']:5.3f}   / linear rebuild {mr / m['r_reb']:5.3f}   / refitted {mr / m['r_ref']:5.3f}")
            print("\n".join(lines[-3 - 2 * len(extra):]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
