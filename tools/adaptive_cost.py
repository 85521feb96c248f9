"""What the rounds of lj_render_adaptive cost beside their renders: the default arguments (min_spp 16, max_spp 256, round_spp 16, 16 rounds,
target_error 0.05) on

    cbox 512 x 512 and sponza at its own film size

After a warm-up, `--rounds` calls each; medians and the spread (min .. max) of the call's render_ms (LjStats: the sum over the rounds'
renders), select_ms and merge_ms (LjAdaptiveStats: sums over the rounds), each also per round, and of the host's share: the wall time of
the call minus those three, per round — the wait for the next list's length, the copy of the list to the host and back, and the launches.

    python tools/adaptive_cost.py [--out profiles/adaptive_cost.txt] [--rounds 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lajolla_public_amd as lj  # noqa: E402

CBOX = os.path.join(ROOT, "scenes", "cbox", "cbox.xml")
SPONZA = os.path.join(ROOT, "scenes", "sponza", "sponza.xml")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    ctx = lj.Context(0)
    med = statistics.median
    cell = lambda t: f"{med(t):9.3f} ({min(t):9.3f} .. {max(t):9.3f})"
    lines = [f"lj_render_adaptive (defaults, rgb + variance + samples to the host), {args.rounds} calls after one warm-up; ms: median (min .. max)"]
    for name, path in [("cbox", CBOX), ("sponza", SPONZA)]:
        sc = lj.Scene(ctx, lj.parse_scene(path))
        w, h = sc.info.width, sc.info.height
        render, select, merge, host = [], [], [], []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            out = lj.render_adaptive(sc)
            wall = (time.perf_counter() - t0) * 1e3
            st, ast = sc.stats(), lj.adaptive_stats(sc)
            if r:
                render.append(st.render_ms); select.append(ast.select_ms); merge.append(ast.merge_ms)
                host.append((wall - st.render_ms - ast.select_ms - ast.merge_ms) / ast.rounds)
        n = int(ast.rounds)
        pixels = [int(ast.round_pixels[r]) for r in range(n)]
        lines.append(f"{name} {w}x{h}: {n} rounds, {int(ast.samples)} samples = {ast.samples / (w * h):.1f} per pixel ({int(out['samples'].min())} .. {int(out['samples'].max())}); round_pixels {pixels}")
        lines.append(f"    render_ms {cell(render)}  per round {med(render) / n:8.3f}")
        lines.append(f"    select_ms {cell(select)}  per round {med(select) / max(n - 1, 1):8.3f} ({n - 1} selections of 3 launches)  = {100 * med(select) / med(render):.2f} % of render_ms")
        lines.append(f"    merge_ms  {cell(merge)}  per round {med(merge) / n:8.3f}  = {100 * med(merge) / med(render):.2f} % of render_ms")
        lines.append(f"    host, per round: wall - render - select - merge {cell(host)}")
        for line in lines[-5:]:
            print(line, flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
