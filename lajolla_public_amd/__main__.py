"""`python -m lajolla_public_amd [-o output_file_name] [--spp N] [--rng tile|sample] [--features] [--denoise] [--adaptive TARGET] [--gpus N | --devices 0,1,..] filename.xml ...` — the reference's
driver loop (main.cpp:12-51) on the HIP path: parse, render, write to `-o` or the scene's own output file name (PFM / EXR).
`-t num_threads` is accepted and ignored (the render does not run on host threads).  `--gpus N` renders on the first N devices of
the node from this one process (a device group: tiles sharded t % N, one RCCL reduce); `--devices` names them (ids may repeat:
logical ranks on one GPU).  `--rng tile` draws the random numbers in the reference's own order (one pcg32 stream per 16x16 tile,
LJ_RNG_TILE: slower, for reproducing a reference render); the default `--rng sample` gives every pixel sample a stream of its own.
`--features` also writes the guide buffers of lj_render_features beside the image, as <stem>.albedo.exr, .normal.exr, .depth.exr, .alpha.exr
and .variance.exr (one-channel buffers replicated to RGB); one device, `--rng sample`, the path and volpath integrators.
`--denoise` also writes <stem>.denoised.exr: the image filtered by lj_denoise over those guide buffers (it renders them, under the conditions
of `--features`, but writes the guide files only with `--features`).
`--adaptive TARGET` renders with lj_render_adaptive: samples in rounds, where the relative error still exceeds TARGET (0: the default, 0.05);
`--spp N` is then the sample count of round 0 and of every later round (up to 16 N per pixel).  It also writes <stem>.samples.exr, the
per-pixel sample counts; one device, `--rng sample`, the path and volpath integrators.  With `--features` and `--denoise` the guide
buffers are those of round 0 and the filter runs on the adaptive image and its variance."""
import os
import sys
import time

from . import _abi
from . import FEATURES, Context, DeviceGroup, GroupScene, Scene, denoise, parse_scene, render, render_adaptive, render_features, render_group, write_image


def main(argv):
    if not argv:
        print("[Usage] python -m lajolla_public_amd [-t num_threads] [-o output_file_name] [--spp N] [--rng tile|sample] [--features] [--denoise] [--adaptive TARGET] [--gpus N | --devices i,j,..] filename.xml")
        return 0
    output, spp, filenames, devices, rng_mode, features, denoised, adaptive = "", 0, [], None, _abi.LJ_RNG_SAMPLE, False, False, None
    i = 0
    while i < len(argv):
        if argv[i] == "-t":
            i += 1
        elif argv[i] == "-o":
            i += 1
            output = argv[i]
        elif argv[i] == "--spp":
            i += 1
            spp = int(argv[i])
        elif argv[i] == "--rng":
            i += 1
            modes = {"sample": _abi.LJ_RNG_SAMPLE, "tile": _abi.LJ_RNG_TILE}
            if argv[i] not in modes:
                print(f"--rng: expected tile or sample, got {argv[i]!r}", file=sys.stderr)
                return 2
            rng_mode = modes[argv[i]]
        elif argv[i] == "--features":
            features = True
        elif argv[i] == "--denoise":
            denoised = True
        elif argv[i] == "--adaptive":
            i += 1
            adaptive = float(argv[i])
        elif argv[i] == "--gpus":
            i += 1
            devices = list(range(int(argv[i])))
        elif argv[i] == "--devices":
            i += 1
            devices = [int(d) for d in argv[i].split(",")]
        else:
            filenames.append(argv[i])
        i += 1
    if features and ((devices and len(devices) > 1) or rng_mode != _abi.LJ_RNG_SAMPLE):
        print("--features: one device and --rng sample only (device groups and the per-tile schedule have no guide buffers)", file=sys.stderr)
        return 2
    if denoised and ((devices and len(devices) > 1) or rng_mode != _abi.LJ_RNG_SAMPLE):
        print("--denoise: one device and --rng sample only (the filter needs the guide buffers, which device groups and the per-tile schedule do not have)", file=sys.stderr)
        return 2
    if adaptive is not None and ((devices and len(devices) > 1) or rng_mode != _abi.LJ_RNG_SAMPLE):
        print("--adaptive: one device and --rng sample only (device groups and the per-tile schedule have no adaptive render)", file=sys.stderr)
        return 2
    group = DeviceGroup(devices) if devices and len(devices) > 1 else None
    ctx = None if group else Context(devices[0] if devices else 0)
    for filename in filenames:
        t0 = time.perf_counter()
        print(f"Parsing and constructing scene {filename}.")
        hs = parse_scene(filename)
        sc = GroupScene(group, hs) if group else Scene(ctx, hs)
        print(f"Done. Took {time.perf_counter() - t0:.6g} seconds.")
        print("Rendering...")
        t0 = time.perf_counter()
        if adaptive is not None:
            buffers = render_adaptive(sc, min_spp=spp, target_error=adaptive, guides=features or denoised)
        else:
            buffers = render_features(sc, spp=spp) if features or denoised else {}
        img = buffers["rgb"] if buffers else (render_group(sc, spp=spp, rng_mode=rng_mode) if group else render(sc, spp=spp, rng_mode=rng_mode))
        if output == "":
            output = hs.desc.output_filename.decode()
        print(f"Done. Took {time.perf_counter() - t0:.6g} seconds.")
        write_image(output, img)
        print(f"Image written to {output}")
        for name in FEATURES if features else ():
            b = buffers[name]
            path = os.path.splitext(output)[0] + "." + name + ".exr"
            write_image(path, b if b.ndim == 3 else b[..., None].repeat(3, axis=-1))
            print(f"{name} written to {path}")
        if adaptive is not None:
            path = os.path.splitext(output)[0] + ".samples.exr"
            write_image(path, buffers["samples"].astype("float32")[..., None].repeat(3, axis=-1))
            print(f"sample counts written to {path}")
        if denoised:
            path = os.path.splitext(output)[0] + ".denoised.exr"
            write_image(path, denoise({k: v for k, v in buffers.items() if k != "samples"}, ctx=ctx)["rgb"])
            print(f"denoised image written to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
