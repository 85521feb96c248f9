"""What the guide buffers cost beside the image: lj_render and lj_render_features (all five buffers) of the same scene and arguments,
alternating, device times from LjStats / LjFeatureStats.

    cbox 512 x 512 at 256 and at 4 spp, disney_bsdf 683 x 512 at 256 spp, sponza 768 x 575 at 256 spp (the scenes' own films)

After a warm-up of both calls, `--rounds` alternating rounds; medians and the spread (min .. max) are reported: render_ms of lj_render, render_ms
of lj_render_features (its timed region also holds the new launches), features_ms (k_features) and variance_ms (k_resolve_variance).
The yardstick: the feature pass traces one coherent closest-hit ray per sample, a render traces rays_closest + rays_shadow rays, so
features_ms / render_ms should not exceed samples / (rays_closest + rays_shadow) of the same render's LjStats.

    python tools/features_cost.py [--out profiles/features_cost.txt] [--rounds 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import lajolla_public_amd as lj  # noqa: E402

CONFIGS = [("cbox", os.path.join(ROOT, "scenes", "cbox", "cbox.xml"), 256),
           ("cbox", os.path.join(ROOT, "scenes", "cbox", "cbox.xml"), 4),
           ("disney_bsdf", os.path.join(ROOT, "scenes", "disney_bsdf_test", "disney_bsdf.xml"), 256),
           ("sponza", os.path.join(ROOT, "scenes", "sponza", "sponza.xml"), 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    ctx = lj.Context(0)
    cell = lambda t: f"{statistics.median(t):8.3f} ({min(t):8.3f} .. {max(t):8.3f})"
    lines = [f"lj_render against lj_render_features (albedo, normal, depth, alpha, variance), {args.rounds} alternating rounds after one warm-up; device ms: median (min .. max)",
             f"{'scene':12s} {'film':9s} {'spp':>4s} {'render_ms (lj_render)':>32s} {'render_ms (features call)':>32s} {'features_ms':>32s} {'variance_ms':>32s}  feat/render  yardstick"]
    for name, path, spp in CONFIGS:
        hs = lj.parse_scene(path)
        sc = lj.Scene(ctx, hs)
        w, h = sc.info.width, sc.info.height
        img = lj.render(sc, spp=spp)                   # warm-up of both calls; the image must be the same
        f = lj.render_features(sc, spp=spp)
        assert np.array_equal(img.view(np.uint32), f["rgb"].view(np.uint32)), "rgb of the features call differs from lj_render"
        plain, with_features, feat, var = [], [], [], []
        yard = 0.0
        for _ in range(args.rounds):
            lj.render(sc, spp=spp)
            st = sc.stats()
            plain.append(st.render_ms)
            yard = st.samples / float(st.rays_closest + st.rays_shadow)
            lj.render_features(sc, spp=spp)
            with_features.append(sc.stats().render_ms)
            fs = lj.feature_stats(sc)
            feat.append(fs.features_ms)
            var.append(fs.variance_ms)
        ratio = statistics.median(feat) / statistics.median(plain)
        lines.append(f"{name:12s} {w:4d}x{h:<4d} {spp:4d} {cell(plain):>32s} {cell(with_features):>32s} {cell(feat):>32s} {cell(var):>32s}  {ratio:11.4f}  {yard:9.4f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
