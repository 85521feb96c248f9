"""What lj_denoise costs beside the render that feeds it: render_features (all buffers) and denoise (defaults: 5 iterations, demodulated) of

    cbox 512 x 512 at 16 spp, disney_bsdf 683 x 512 at 16 spp, and a batch of 16 views of cbox at 256 x 256 and 16 spp

After a warm-up, `--rounds` calls each; medians and the spread (min .. max) of render_ms (LjStats of the features call) and denoise_ms
(LjDenoiseStats: pack + iterations + unpack).  Per-iteration device time: denoise_ms at k iterations minus denoise_ms at k - 1 (medians);
the time of 1 iteration + pack + unpack is listed as one figure.
Beside each, the derived floor of an iteration: (64 B read + 32 B written) * n * h * w at 6.29 TB/s (the measured float4 copy rate of the
HBM), the launches, and the regime that floor puts the frame in.
The same table once per LJ_TUNE_DENOISE_LDS setting (0: all direct .. 3: steps 1, 2 and 4 from LDS).

    python tools/denoise_cost.py [--out profiles/denoise_cost.txt] [--rounds 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lajolla_public_amd as lj  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
CBOX = os.path.join(ROOT, "scenes", "cbox", "cbox.xml")
DISNEY = os.path.join(ROOT, "scenes", "disney_bsdf_test", "disney_bsdf.xml")


def cbox_views(n, size):
    return [lj.look_at_camera((278 + 12 * (v - n / 2), 273, -800), (278, 273, 0), (0, 1, 0), 39.3077, size, size) for v in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    ctx = lj.Context(0)
    med = statistics.median
    cell = lambda t: f"{med(t):7.3f} ({min(t):7.3f} .. {max(t):7.3f})"
    lines = [f"lj_render_features (all buffers) and lj_denoise (defaults, demodulated), {args.rounds} calls after one warm-up; device ms: median (min .. max)"]
    for name, path, n, size, spp in [("cbox", CBOX, 1, None, 16), ("disney_bsdf", DISNEY, 1, None, 16), ("cbox x16", CBOX, 16, 256, 16)]:
        sc = lj.Scene(ctx, lj.parse_scene(path))
        cams = None
        if size:
            cams = cbox_views(n, size)
            sc.set_camera(cams[0])
        w, h = sc.info.width, sc.info.height
        render = []
        for r in range(args.rounds + 1):
            b = lj.render_features(sc, cameras=cams, spp=spp)
            if r:
                render.append(sc.stats().render_ms)
        pixels = n * w * h
        floor_ms = 96.0 * pixels / HBM_BYTES_PER_S * 1e3
        regime = "floor under 20 us: launches, latency and arithmetic set the time, not HBM" if floor_ms < 0.02 else "HBM bandwidth can bound it"
        lines.append(f"{name:12s} {n:2d} x {w}x{h} @ {spp} spp: render_ms {cell(render)}; floor per iteration {floor_ms:.4f} ms ({96 * pixels / 1e6:.1f} MB), 5 iterations + pack + unpack "
                     f"= 7 launches; {regime}")
        for lds in (0, 1, 2, 3):
            os.environ["LJ_TUNE_DENOISE_LDS"] = str(lds)
            totals = []
            for it in (1, 2, 3, 4, 5):
                t = []
                for r in range(args.rounds + 1):
                    lj.denoise(b, ctx=ctx, iterations=it)
                    if r:
                        t.append(lj.denoise_stats(ctx).denoise_ms)
                totals.append(t)
            per_it = [med(totals[k]) - med(totals[k - 1]) for k in range(1, 5)]
            lines.append(f"    LJ_TUNE_DENOISE_LDS={lds}: denoise_ms {cell(totals[4])} = {med(totals[4]) / med(render):6.3f} of render_ms; 1 iteration + pack + unpack {med(totals[0]):.3f}; "
                         f"iterations 2..5 (steps 2, 4, 8, 16): " + ", ".join(f"{x:.3f}" for x in per_it) + f"; floor x{(med(totals[4]) / (5 * floor_ms)):.1f}")
            print(lines[-1], flush=True)
        del os.environ["LJ_TUNE_DENOISE_LDS"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
