"""Build liblajolla_hip.so (product) — and, for the test infrastructure, oracle/_build/liblj_oracle.so.

    python -m lajolla_public_amd.build            # product library (hipcc --offload-arch=gfx950, cross-compiles without a GPU)
    python -m lajolla_public_amd.build --oracle   # also the CPU oracle (g++), test infrastructure only
    python -m lajolla_public_amd.build --twin     # also the host build of the device headers used by CPU-side tests

Objects are cached under build/ and rebuilt when a source or header is newer.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lajolla_public_amd", "csrc")
# LJ_VARIANT=name (developer A/B runs, tools/ab.sh): a second library beside the default one, built with
# LJ_EXTRA_HIPCC_FLAGS into its own object directory and picked up by the package when LJ_VARIANT is set at import
_VARIANT = os.environ.get("LJ_VARIANT", "")
BUILD = os.path.join(ROOT, "build" + ("_" + _VARIANT if _VARIANT else ""))
LIB = os.path.join(ROOT, "lajolla_public_amd", "liblajolla_hip" + ("_" + _VARIANT if _VARIANT else "") + ".so")
# LJ_SANITIZE=1 (tools/sanitize_cpu.sh): AddressSanitizer + UndefinedBehaviorSanitizer builds of the two CPU-side test libraries
# (the GPU pool offers no device sanitizer; the host twin compiles the very device headers, so it is the next best thing)
_SAN = bool(os.environ.get("LJ_SANITIZE"))
_SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if _SAN else []
ORACLE_LIB = os.path.join(ROOT, "oracle", "_build", "liblj_oracle_asan.so" if _SAN else "liblj_oracle.so")
TWIN_LIB = os.path.join(ROOT, "tests", "twin", "_build", "libljtwin_asan.so" if _SAN else "libljtwin.so")

HOST_SOURCES = ["host/api_host.cpp", "host/scene_xml.cpp", "host/mesh_io.cpp", "host/image_io.cpp", "host/jpeg_decode.cpp", "host/exr_decode.cpp", "host/png_decode.cpp", "host/tga_bmp_decode.cpp", "host/flatten.cpp", "host/bvh.cpp"]
HIP_SOURCES = ["device/kernels.hip", "device/shade_rays.hip", "device/volpath.hip", "device/extend.hip", "device/extend8.hip", "device/api_device.hip", "device/api_geometry.hip", "device/api_film.hip", "device/api_denoise.hip", "device/api_rays.hip", "device/render.hip", "device/queries.hip", "device/mega.hip", "device/group.hip", "device/tile.hip", "device/refit.hip", "device/features.hip", "device/denoise.hip", "device/adaptive.hip", "device/rebuild.hip", "device/ploc.hip"]
ARCH = "gfx950"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _headers():
    out = [os.path.join(ROOT, "include", "lajolla_hip.h")]
    for d, _, files in os.walk(CSRC):
        out += [os.path.join(d, f) for f in files if f.endswith(".h")]
    return out


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: " + " ".join(cmd) + "\n" + r.stdout)
    if r.stdout.strip():
        sys.stderr.write(r.stdout)
    # the command line is part of an object's cache key (a sidecar next to it): a build with other flags — e.g.
    # LJ_EXTRA_HIPCC_FLAGS from tools/occ_sweep.sh — is rebuilt by the next default build instead of being silently reused
    if "-o" in cmd:
        with open(cmd[cmd.index("-o") + 1] + ".cmd", "w") as f:
            f.write(" ".join(cmd))


def _same_cmd(target, cmd):
    try:
        return open(target + ".cmd").read() == " ".join(cmd)
    except OSError:
        return False


def build_product(verbose=True):
    if os.environ.get("LJ_NO_REBUILD") and os.path.exists(LIB):   # developer A/B runs of a prebuilt LJ_VARIANT library on the GPU box
        return LIB
    # Extra compiler flags make a VARIANT of the library (developer A/B runs).  They may only go into a library of their own
    # (LJ_VARIANT=name -> liblajolla_hip_<name>.so) — never silently into the default one, where the next test run would load them.
    if os.environ.get("LJ_EXTRA_HIPCC_FLAGS") and not _VARIANT and os.environ.get("LJ_VARIANT_OK") != "1":
        raise RuntimeError("LJ_EXTRA_HIPCC_FLAGS is set without LJ_VARIANT: refusing to build the default library with variant flags "
                           "(set LJ_VARIANT=<name> for a side-by-side library, or LJ_VARIANT_OK=1 to override)")
    os.makedirs(BUILD, exist_ok=True)
    headers = _headers()
    jobs = []
    objs = []
    for src in HOST_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(BUILD, src.replace("/", "_") + ".o")
        objs.append(o)
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-Wall", "-Wno-unused-function", "-c", s, "-o", o]
        if _stale(o, [s] + headers) or not _same_cmd(o, cmd):
            jobs.append(cmd)
    for src in HIP_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(BUILD, src.replace("/", "_") + ".o")
        objs.append(o)
        # -fno-slp-vectorize: packed-fp32 pairs (v_pk_add/mul/fma_f32) cost more in register shuffling than they save
        # in these kernels (measured: -6 % cbox, -14 % veach_mi, -1..4 % elsewhere; 12 fewer VGPRs in the extend kernel)
        # (not built with -fno-hip-fp32-correctly-rounded-divide-sqrt: the 2.5-ulp divisions are 2 % faster on every scene, but the
        # volumetric tracker's long chains of accept / reject decisions then leave the oracle's path in most samples of a dense medium —
        # vol_cbox per-sample parity went from a median 2e-7 to 0.15 — and sponza's per-sample median crossed its 1e-4 bar: measured, dropped)
        cmd = [_hipcc(), "-std=c++17", "-O3", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
               "-fno-gpu-rdc", "-fno-slp-vectorize"] + os.environ.get("LJ_EXTRA_HIPCC_FLAGS", "").split() + ["-c", s, "-o", o]
        # (shade_rays.hip is compiled from the templates of kernels.hip, which it includes)
        included = [os.path.join(CSRC, "device/kernels.hip")] if src == "device/shade_rays.hip" else []
        if _stale(o, [s] + included + headers) or not _same_cmd(o, cmd):
            jobs.append(cmd)
    if jobs:
        if verbose:
            print(f"[build] compiling {len(jobs)} translation unit(s) for {ARCH}", file=sys.stderr)
        with ThreadPoolExecutor(max_workers=4) as ex:
            list(ex.map(_run, jobs))
    if jobs or _stale(LIB, objs):
        _run([_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB] + objs + ["-lz"])
    return LIB


def _host_fma_flag():
    """-mfma when this CPU has it: the oracle's explicit fmaf() calls then compile to one instruction instead of a libm
    call (same result either way — fma is exactly specified)."""
    try:
        return ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    except OSError:
        return []


def build_oracle(verbose=True):
    src = os.path.join(ROOT, "oracle", "lj_oracle.cpp")
    os.makedirs(os.path.dirname(ORACLE_LIB), exist_ok=True)
    if _stale(ORACLE_LIB, [src, os.path.join(ROOT, "include", "lajolla_hip.h")]):
        if verbose:
            print("[build] compiling the CPU oracle (test infrastructure)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", ORACLE_LIB, src, "-lpthread"])
    return ORACLE_LIB


def build_twin(verbose=True):
    src = os.path.join(ROOT, "tests", "twin", "twin.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the device headers (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_LIB


TWIN_TILE_LIB = os.path.join(ROOT, "tests", "twin_tile", "_build", "libljtwintile_asan.so" if _SAN else "libljtwintile.so")


def build_twin_tile(verbose=True):
    """Host build of the per-tile schedule (device/dtile.h) for the CPU-side tests of LJ_RNG_TILE; the flags of build_twin."""
    src = os.path.join(ROOT, "tests", "twin_tile", "twin_tile.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_TILE_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_TILE_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the per-tile schedule (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_TILE_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_TILE_LIB


TWIN_REGEN_LIB = os.path.join(ROOT, "tests", "twin_regen", "_build", "libljtwinregen_asan.so" if _SAN else "libljtwinregen.so")


def build_twin_regen(verbose=True):
    """Host model of a persistent k_mega grid over the kernel's sample bookkeeping (device/dregen.h) for the CPU-side tests."""
    src = os.path.join(ROOT, "tests", "twin_regen", "twin_regen.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_REGEN_LIB), exist_ok=True)
    if _stale(TWIN_REGEN_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host model of the mega kernel's sample bookkeeping (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2"] + _SAN_FLAGS + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", TWIN_REGEN_LIB, src])
    return TWIN_REGEN_LIB


TWIN_POOL_LIB = os.path.join(ROOT, "tests", "twin_pool", "_build", "libljtwinpool_asan.so" if _SAN else "libljtwinpool.so")


def build_twin_pool(verbose=True):
    """Host model of one k_mega wave's candidate pool over the kernel's pass arithmetic (device/dmegapool.h) for the CPU-side tests."""
    src = os.path.join(ROOT, "tests", "twin_pool", "twin_pool.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_POOL_LIB), exist_ok=True)
    if _stale(TWIN_POOL_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host model of the mega kernel's candidate pool (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2"] + _SAN_FLAGS + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", TWIN_POOL_LIB, src])
    return TWIN_POOL_LIB


TWIN_ROUND_LIB = os.path.join(ROOT, "tests", "twin_round", "_build", "libljtwinround_asan.so" if _SAN else "libljtwinround.so")


def build_twin_round(verbose=True):
    """Host model of the test rounds of a k_mega pass, the split of a short last round included (device/dmegapool.h), for the CPU-side tests."""
    src = os.path.join(ROOT, "tests", "twin_round", "twin_round.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_ROUND_LIB), exist_ok=True)
    if _stale(TWIN_ROUND_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host model of the mega kernel's test rounds (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2"] + _SAN_FLAGS + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", TWIN_ROUND_LIB, src])
    return TWIN_ROUND_LIB


TWIN_SCAN_LIB = os.path.join(ROOT, "tests", "twin_scan", "_build", "libljtwinscan_asan.so" if _SAN else "libljtwinscan.so")


def build_twin_scan(verbose=True):
    """Host build of the leaf scan's box arithmetic and table conversion (device/dscan.h) for the CPU-side tests."""
    src = os.path.join(ROOT, "tests", "twin_scan", "twin_scan.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_SCAN_LIB), exist_ok=True)
    if _stale(TWIN_SCAN_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host twin of the leaf scan's box test (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_SCAN_LIB, src])
    return TWIN_SCAN_LIB


TWIN_VIEWS_LIB = os.path.join(ROOT, "tests", "twin_views", "_build", "libljtwinviews_asan.so" if _SAN else "libljtwinviews.so")


def build_twin_views(verbose=True):
    """Host build of the camera-batch path of the device headers (DPass::views: lj_render_views) for the CPU-side tests; the flags of build_twin."""
    src = os.path.join(ROOT, "tests", "twin_views", "twin_views.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_VIEWS_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_VIEWS_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the camera-batch path (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_VIEWS_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_VIEWS_LIB


TWIN_REFIT_LIB = os.path.join(ROOT, "tests", "twin_refit", "_build", "libljtwinrefit_asan.so" if _SAN else "libljtwinrefit.so")


def build_twin_refit(verbose=True):
    """Host twin of lj_scene_update_geometry (flatten_update and the refit of device/drefit.h) for the CPU-side tests; the flags of build_twin."""
    src = os.path.join(ROOT, "tests", "twin_refit", "twin_refit.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_REFIT_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_REFIT_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the geometry update and refit (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_REFIT_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_REFIT_LIB


TWIN_FEATURES_LIB = os.path.join(ROOT, "tests", "twin_features", "_build", "libljtwinfeatures_asan.so" if _SAN else "libljtwinfeatures.so")


def build_twin_features(verbose=True):
    """Host build of the guide-buffer path of the device headers (device/dfeature.h: lj_render_features) for the CPU-side tests; the flags of build_twin."""
    src = os.path.join(ROOT, "tests", "twin_features", "twin_features.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_FEATURES_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_FEATURES_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the guide-buffer path (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_FEATURES_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_FEATURES_LIB


TWIN_DENOISE_LIB = os.path.join(ROOT, "tests", "twin_denoise", "_build", "libljtwindenoise_asan.so" if _SAN else "libljtwindenoise.so")


def build_twin_denoise(verbose=True):
    """Host build of the filter of lj_denoise (device/ddenoise.h) for the CPU-side tests; the flags of build_twin_features, and no scene source."""
    src = os.path.join(ROOT, "tests", "twin_denoise", "twin_denoise.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_DENOISE_LIB), exist_ok=True)
    if _stale(TWIN_DENOISE_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host twin of the denoising filter (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_DENOISE_LIB, src])
    return TWIN_DENOISE_LIB


TWIN_ADAPTIVE_LIB = os.path.join(ROOT, "tests", "twin_adaptive", "_build", "libljtwinadaptive_asan.so" if _SAN else "libljtwinadaptive.so")


def build_twin_adaptive(verbose=True):
    """Host build of the rule of lj_render_adaptive (device/dadaptive.h) for the CPU-side tests; the flags of build_twin_denoise, and no scene source."""
    src = os.path.join(ROOT, "tests", "twin_adaptive", "twin_adaptive.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_ADAPTIVE_LIB), exist_ok=True)
    if _stale(TWIN_ADAPTIVE_LIB, [src] + _headers()):
        if verbose:
            print("[build] compiling the host twin of the adaptive-sampling rule (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_ADAPTIVE_LIB, src])
    return TWIN_ADAPTIVE_LIB


TWIN_REBUILD_LIB = os.path.join(ROOT, "tests", "twin_rebuild", "_build", "libljtwinrebuild_asan.so" if _SAN else "libljtwinrebuild.so")


def build_twin_rebuild(verbose=True):
    """Host twin of lj_scene_rebuild_bvh (the build rule of device/drebuild.h, emit_wide, and the twin of the geometry update it includes) for
    the CPU-side tests; the flags of build_twin_refit."""
    src = os.path.join(ROOT, "tests", "twin_rebuild", "twin_rebuild.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_REBUILD_LIB), exist_ok=True)
    deps = [src, os.path.join(ROOT, "tests", "twin_refit", "twin_refit.cpp")] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_REBUILD_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the BVH rebuild (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_REBUILD_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_REBUILD_LIB


TWIN_PLOC_LIB = os.path.join(ROOT, "tests", "twin_ploc", "_build", "libljtwinploc_asan.so" if _SAN else "libljtwinploc.so")


def build_twin_ploc(verbose=True):
    """Host twin of lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC (the rule of device/dploc.h, compact_ploc_tree, and the twin of the rebuild it
    includes) for the CPU-side tests; the flags of build_twin_rebuild."""
    src = os.path.join(ROOT, "tests", "twin_ploc", "twin_ploc.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_PLOC_LIB), exist_ok=True)
    deps = [src, os.path.join(ROOT, "tests", "twin_rebuild", "twin_rebuild.cpp"), os.path.join(ROOT, "tests", "twin_refit", "twin_refit.cpp")] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_PLOC_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the PLOC rebuild (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_PLOC_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_PLOC_LIB


TWIN_RAYS_LIB = os.path.join(ROOT, "tests", "twin_rays", "_build", "libljtwinrays_asan.so" if _SAN else "libljtwinrays.so")


def build_twin_rays(verbose=True):
    """Host build of the ray source of the device headers (device/dprobe.h: lj_radiance_rays, lj_irradiance) for the CPU-side tests; the flags of build_twin."""
    src = os.path.join(ROOT, "tests", "twin_rays", "twin_rays.cpp")
    if not os.path.exists(src):
        return None
    os.makedirs(os.path.dirname(TWIN_RAYS_LIB), exist_ok=True)
    deps = [src] + _headers() + [os.path.join(CSRC, s) for s in ("host/flatten.cpp", "host/bvh.cpp")]
    if _stale(TWIN_RAYS_LIB, deps):
        if verbose:
            print("[build] compiling the host twin of the ray source (CPU-side tests only)", file=sys.stderr)
        _run(["g++", "-std=c++17", "-O1" if _SAN else "-O2", "-ffp-contract=off"] + _SAN_FLAGS + _host_fma_flag() + ["-fPIC", "-shared", "-Wall", "-Wno-unused-function",
              "-o", TWIN_RAYS_LIB, src, os.path.join(CSRC, "host/flatten.cpp"), os.path.join(CSRC, "host/bvh.cpp"), "-lpthread"])
    return TWIN_RAYS_LIB


def build_reference_subset():
    """oracle/_ref from the reference's own sources — only where /root/reference exists (this container)."""
    script = os.path.join(ROOT, "oracle", "ref_build.sh")
    if os.path.isdir(os.environ.get("LJ_REFERENCE_ROOT", "/root/reference")):
        _run(["bash", script])


if __name__ == "__main__":
    build_product()
    if "--oracle" in sys.argv or "--all" in sys.argv:
        build_oracle()
    if "--twin" in sys.argv or "--all" in sys.argv:
        build_twin()
        build_twin_tile()
        build_twin_regen()
        build_twin_pool()
        build_twin_round()
        build_twin_scan()
        build_twin_views()
        build_twin_refit()
        build_twin_features()
        build_twin_denoise()
        build_twin_adaptive()
        build_twin_rebuild()
        build_twin_ploc()
        build_twin_rays()
    print(LIB)
