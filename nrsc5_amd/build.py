"""Build recipe for libnrsc5hip.so (hipcc, gfx950 only).  `python -m nrsc5_amd.build`.

The CPU-emulated twin used by the `-m "not gpu"` logic tests is built by `build_emu()` into
tests/simt/ -- test infrastructure, never loaded by the package itself."""
from __future__ import annotations

import contextlib
import fcntl
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrsc5_amd", "csrc")
HIP_SOURCES = ["engine.hip", "engine_steps.hip", "engine_seam.hip", "engine_batch.hip", "engine_stage.hip", "k_decimate.hip", "k_acquire.hip", "k_mixfft.hip", "k_sync.hip", "k_pids_px.hip", "k_decode.hip", "k_replay.hip", "k_trim.hip", "k_am_decimate.hip", "k_am.hip", "k_am_decode.hip", "k_l2.hip", "hdc_consumer.hip", "k_psd.hip", "psd_consumer.hip", "k_sis.hip", "sis_consumer.hip", "k_aas.hip", "aas_consumer.hip", "k_channelize.hip", "k_scan.hip", "k_fm_audio.hip", "fm_audio.hip", "k_fm_carrier.hip", "fm_carrier.hip", "k_fm_impair.hip", "fm_impair.hip", "k_rds.hip", "rds.hip", "k_same.hip", "same.hip"]
LIB = os.path.join(ROOT, "nrsc5_amd", "libnrsc5hip.so")
EMU_LIB = os.path.join(ROOT, "tests", "simt", "libnrsc5hip_emu.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps():
    d = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    d.append(os.path.join(ROOT, "include", "nrsc5hip.h"))
    return d


@contextlib.contextmanager
def _build_lock(target: str):
    """Serialises builds of one output across processes (pytest-xdist workers start together on a clean checkout): the caller checks
    again, under the lock, whether the output is still stale, since another process may have built it meanwhile."""
    fd = os.open(os.path.dirname(target), os.O_RDONLY)
    try:
        fcntl.flock(fd, fcntl.LOCK_EX)
        yield
    finally:
        os.close(fd)


def _compile_to(target: str, cmd_for) -> None:
    """Runs cmd_for(path) with a temporary path next to target, then replaces target in one rename: a process that has the old library
    mapped, or opens it meanwhile, never sees a half-written file."""
    tmp = "%s.tmp%d" % (target, os.getpid())
    try:
        subprocess.check_call(cmd_for(tmp))
        os.replace(tmp, target)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


def source_sha() -> str:
    """Fingerprint of the device sources: measurements stored under profiles/ carry it, so that bench.py can tell whether a PMC
    figure was collected from THIS tree."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(_deps()):
        if f.endswith((".hip", ".h")):
            h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def build_hip(force: bool = False, verbose: bool = False) -> str:
    """Cross-compiles on a GPU-less host too (hipcc --offload-arch=gfx950)."""
    if force or _stale(LIB, _deps()):
        with _build_lock(LIB):
            if force or _stale(LIB, _deps()):                   # not built by another process while this one waited
                srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES if os.path.exists(os.path.join(CSRC, f))]

                def cmd(out):
                    c = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                         '-DNRSC5HIP_SOURCE_SHA="%s"' % source_sha(),        # nrsc5hip_source_sha(): callers can tell a stale build from the tree they run in
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out] + srcs
                    if verbose:
                        print(" ".join(c))
                    return c
                _compile_to(LIB, cmd)
    return LIB


def build_hip_diag(flags, out_name: str) -> str:
    """A diagnostic twin of the library with extra -D flags (e.g. -DNRSC5HIP_MIXFFT_PHASES: k_mixfft's phase timers), same sources and
    fingerprint, written next to the release library under its own name; tools/ scripts load it by path."""
    out = os.path.join(ROOT, "nrsc5_amd", out_name)
    srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES if os.path.exists(os.path.join(CSRC, f))]
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", '-DNRSC5HIP_SOURCE_SHA="%s"' % source_sha(),
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out] + list(flags) + srcs
    subprocess.check_call(cmd)
    return out


def _host_has_fma() -> bool:
    try:
        flags = next(l for l in open("/proc/cpuinfo") if l.startswith("flags")).split()
    except (OSError, StopIteration):
        return False
    return "fma" in flags


def build_emu(force: bool = False) -> str:
    simt = os.path.join(ROOT, "tests", "simt")
    deps = _deps() + [os.path.join(simt, "hipemu.h"), os.path.join(simt, "hipemu.cpp")]
    if force or _stale(EMU_LIB, deps):
        with _build_lock(EMU_LIB):
            if force or _stale(EMU_LIB, deps):                  # not built by another process while this one waited
                srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES if os.path.exists(os.path.join(CSRC, f))]
                # -mfma (where the host has it): __builtin_fma of ref_sincosf becomes the instruction instead of a libm call; -ffp-contract=off keeps every other a * b + c unfused
                fma = ["-mfma"] if _host_has_fma() else []

                def cmd(out):
                    c = ["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w"] + fma + ['-DNRSC5HIP_SOURCE_SHA="%s"' % source_sha(),
                         "-I" + simt, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", out,
                         os.path.join(simt, "hipemu.cpp")]
                    for s in srcs:
                        c += ["-x", "c++", s]
                    return c
                _compile_to(EMU_LIB, cmd)
    return EMU_LIB


if __name__ == "__main__":
    if "--emu" in sys.argv:
        print(build_emu(force=True))
    elif "--accurate-trig" in sys.argv:
        print(build_hip_diag(["-DNRSC5HIP_ACCURATE_TRIG"], "libnrsc5hip_acctrig.so"))
    elif "--cmul-unfused" in sys.argv:
        print(build_hip_diag(["-DNRSC5HIP_CMUL_UNFUSED"], "libnrsc5hip_unfused.so"))
    elif "--mixfft-noload" in sys.argv:
        print(build_hip_diag(["-DNRSC5HIP_MIXFFT_NOLOAD"], "libnrsc5hip_noload.so"))
    elif "--mixfft-phases" in sys.argv:
        print(build_hip_diag(["-DNRSC5HIP_MIXFFT_PHASES"], "libnrsc5hip_mixphases.so"))
    elif "--tbwalk-phases" in sys.argv:
        print(build_hip_diag(["-DNRSC5HIP_TBWALK_PHASES"], "libnrsc5hip_tbphases.so"))
    else:
        print(build_hip(force=True, verbose=True))
