"""Runs the checks of tests/halfband_checks.py on the gfx950 library and writes what they compared to profiles/halfband_raw_stage.txt:
outputs per form and set, all equal or the first mismatches, and the rounding / denormal probe values seen.
    python tools/gpu_halfband_raw_stage.py [output file]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from nrsc5_amd import build, engine
    from oracle import port
    from tests import halfband_args as ha, halfband_checks as hc
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "halfband_raw_stage.txt")
    lib = build.build_hip()
    E = hc.make_engine(lib)
    oracle = port.Oracle()
    report = ["nrsc5hip_stage_halfband_raw on the device against oracle.halfband_fm_cu8 (source %s)" % engine.library_sha(lib),
              "per set: %d requests x leads %s; nearest-mode probes are 0x%08x (rounding) and 0x%08x (denormal)"
              % (len(ha.requests("const0")), ha.LEADS, hc.PROBE_NEAREST, hc.PROBE_DENORMAL), ""]
    failed = []
    for name in ha.SET_NAMES:
        try:
            hc.check_set(E, oracle, name, report)
        except AssertionError as err:
            failed.append(name)
            report.append("FAILED %s: %s" % (name, str(err).split("\n")[0]))
    report.append("HB_ACQ contiguous span from sample 0: %d outputs, all equal" % hc.check_acq_span(E, oracle))
    report.append("")
    report.append("sets failed: %s" % (", ".join(failed) if failed else "none"))
    E.close()
    open(out, "w").write("\n".join(report) + "\n")
    print("\n".join(report))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
