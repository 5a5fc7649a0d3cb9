"""The checks of the analog FM demodulator (nrsc5hip_fm_*, nrsc5_amd/csrc/k_fm_audio.hip), written once and run twice: by
tests/test_fm_stage_cpu.py on the CPU-emulated twin (numpy buffers passed by address) and by tests/test_gpu_fm_stage.py on gfx950 (torch
tensors on the device).  The reference is the float64 restatement tests/fm_model.py on the inputs of tests/fm_args.py.

Bounds.  Audio: no sample more than 1 LSB from the float64 model, at most 1 % of the samples different (the channelizer's bound,
tests/test_wideband_cpu.py); the float32 model, the reference's own estimate of that share, stays under 0.5 % on every input (asserted in
fm_args.reference).  d through the stage hook: 4 x the largest |float32 model - float64 model| of the same input; on the twelve inputs with a
carrier that largest difference is 2.3e-7 .. 7.3e-7 (d is of order 1: a few float32 ulps), so the bound is 9.3e-7 .. 2.9e-6, and the library
(twin and gfx950 alike) is within 4.6e-7 .. 6.1e-7 -- the margin is there because the library sums the taps in another order and its atan2
is glibc's float one, not numpy's.  Inputs without a carrier are not compared: on noise alone the discriminator is ill-conditioned."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng
from tests import fm_args as fa, fm_model as fm


class Backend:
    """where buffers live: host memory for the twin, the device for the real library"""

    def __init__(self, lib_path: str, gpu: bool):
        self.lib_path, self.gpu = lib_path, gpu

    def demod(self, nchan: int, **kw):
        return eng.FmDemod(nchan, lib_path=self.lib_path, **kw)

    def upload(self, a: np.ndarray):
        """-> (keep-alive object, address)"""
        a = np.ascontiguousarray(a)
        if not self.gpu:
            return a, a.ctypes.data
        import torch
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        return t, t.data_ptr()

    def zeros(self, shape):
        if not self.gpu:
            a = np.zeros(shape, dtype=np.int16)
            return a, a.ctypes.data
        import torch
        t = torch.zeros(shape, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        return t, t.data_ptr()

    def download(self, obj) -> np.ndarray:
        return obj.cpu().numpy() if self.gpu else obj


def stack(names) -> np.ndarray:
    return np.stack([fa.host(n) for n in names])


def run(be: Backend, D, x: np.ndarray, chunks):
    """push x (int16 [K, n, 2]) in the given chunk sizes (the last one takes the rest) -> (pcm int16 [K, frames, 2], clips [K, 2]); every call's
    count is checked against outputs_for"""
    k, n = x.shape[0], x.shape[1]
    assert k == D.nchan
    keep_in, p_in = be.upload(x)
    cap = fm.outputs_total(n) + 64
    keep_out, p_out = be.zeros((k, cap, 2))
    pos = got = 0
    chunks = list(chunks) + [n]
    for c in chunks:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        want = D.outputs_for(c)
        g = D.process(p_in + 4 * pos, 2 * n, c, p_out + 4 * got, 2 * cap, cap - got)
        assert g == want and g % fm.BLOCK_OUT == 0
        pos += c
        got += g
    assert pos == n and got == fm.outputs_total(n)
    return be.download(keep_out)[:, :got].copy(), D.clip_counts()


def compare(got: np.ndarray, clips, name: str, gain=None) -> float:
    """one channel against the float64 model -> the share of samples that differ"""
    want, want_clips, _ = fa.reference(name, gain)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float(np.mean(diff != 0))
    print(f"{name}: largest difference {diff.max()} LSB, {100 * share:.4f} % of the samples differ (float32 model: {100 * fa.reference(name, gain)[2]['share32']:.4f} %), "
          f"rms {np.sqrt(np.mean(want.astype(np.float64) ** 2)):.0f} LSB, clips {list(clips)}")
    assert diff.max() <= 1, (name, diff.max())
    assert share <= 0.01, (name, share)
    assert np.array_equal(np.asarray(clips), want_clips), (name, clips, want_clips)
    return share


# ------------------------------------------------------------------------------------------------------------------ filter responses
def check_filter_responses(be: Backend):
    for de in (75.0, 50.0, 0.0):
        D = be.demod(1, deemphasis_us=de)
        ha, tab = D.tables()
        assert ha.shape == (fm.TA,) == (D.taps_channel,) and tab.shape == (fm.PHASES, D.taps_audio) and D.phases == fm.PHASES
        assert D.latency_in == fm.LATENCY_IN
        mha, mtab = fa.tables(de)
        assert tab.shape == mtab.shape
        assert np.max(np.abs(ha.astype(np.float64) - fm.design_ha())) <= 2.0 ** -24 * np.max(np.abs(ha))          # equal to float32 rounding
        assert np.max(np.abs(tab.astype(np.float64) - fm.design_audio(de))) <= 2.0 ** -24 * np.max(np.abs(tab))
        # channel filter: +-0.1 dB to 95 kHz, >= 70 dB from the first primary-main carrier
        h = ha.astype(np.float64)
        pdb = fm.response_db(h, np.linspace(0.0, 95e3, 600), fm.FS)
        sdb = fm.response_db(h, np.linspace(129361.0, fm.FS / 2, 3000), fm.FS)
        assert np.max(np.abs(pdb)) <= 0.1 and np.max(sdb) <= -70.0, (np.max(np.abs(pdb)), np.max(sdb))
        # audio prototype at 16 Fs1: the de-emphasis curve to 15 kHz, >= 60 dB from 19 kHz to the virtual Nyquist frequency
        g = fm.prototype(tab)
        nfft = 1 << 19
        H = np.abs(np.fft.rfft(g, nfft))
        fr = np.arange(H.size) * (fm.PHASES * fm.FS1) / nfft
        db = 20 * np.log10(np.maximum(H / H[0], 1e-30))
        want = -10 * np.log10(1 + (2 * np.pi * fr * de * 1e-6) ** 2)
        pb = fr <= 15e3
        assert pb.sum() > 1000 and np.max(np.abs(db[pb] - want[pb])) <= 0.1, np.max(np.abs(db[pb] - want[pb]))
        assert np.max(db[fr >= 19e3]) <= -60.0, np.max(db[fr >= 19e3])
        assert abs(g.sum() - fm.PHASES) < 1e-4                                 # DC gain 1 per phase
        print(f"deemphasis {de:g}: hA passband {np.max(np.abs(pdb)):.4f} dB stopband {np.max(sdb):.1f} dB; audio {D.taps_audio} taps x 16, "
              f"passband error {np.max(np.abs(db[pb] - want[pb])):.4f} dB, stopband {np.max(db[fr >= 19e3]):.1f} dB")
        D.close()


# --------------------------------------------------------------------------------------------------------- audio against the model
def check_audio_case(be: Backend, name: str) -> float:
    D = be.demod(1, **fa.demod_args(name))
    got, clips = run(be, D, stack([name]), [])
    D.close()
    return compare(got[0], clips[0], name)


def check_audio_multi(be: Backend, k: int) -> list:
    """K channels with different programmes, and a gain of its own for the last one"""
    names = fa.MULTI[k]
    gains = [1.0] * (k - 1) + [0.5 if k > 1 else 1.0]
    D = be.demod(k, gains=gains)
    got, clips = run(be, D, stack(names), [50000])
    D.close()
    return [compare(got[c], clips[c], names[c], gains[c]) for c in range(k)]


# ----------------------------------------------------------------------------------------------------- d through the stage hook
def check_stage_d(be: Backend, names=None):
    names = list(names or fa.CARRIER_CASES)
    names = [n for n in names if "gain" not in fa.CASES[n][1]]                  # (gain4 is l1k's input again)
    D = be.demod(len(names))
    keep, ptr = be.upload(stack(names))
    d, p = D.stage_mpx(ptr, 2 * fa.N, fa.N)
    D.close()
    assert d.shape == (len(names), fa.N // 2) and p.shape == (len(names), fa.N // 2 // fm.BLOCK)
    for c, name in enumerate(names):
        _, _, info = fa.reference(name)
        tol_d, tol_p = 4 * info["d_err32"], 4 * info["p_err32"]
        err_d = np.max(np.abs(d[c].astype(np.float64) - info["d"]))
        err_p = np.max(np.abs(p[c].astype(np.complex128) - info["psum"]))
        print(f"{name}: d within {err_d:.3g} of the float64 model (bound {tol_d:.3g}), block sums within {err_p:.3g} (bound {tol_p:.3g})")
        assert 1e-7 < info["d_err32"] < 2e-6                                    # the bound is a few float32 ulps of a quantity of order 1
        assert err_d <= tol_d, (name, err_d, tol_d)
        assert err_p <= tol_p, (name, err_p, tol_p)
        assert d[c, 0] == 0.0 and np.all(np.isfinite(d[c]))


# ---------------------------------------------------------------------------------------------------------------------- chunking
def chunk_plans(n: int):
    rng = np.random.default_rng(1080)
    return {"sevens": [7] * (n // 7 + 1), "1079": [1079] * (n // 1079 + 1), "1080": [1080] * (n // 1080 + 1), "1081": [1081] * (n // 1081 + 1),
            "random": list(rng.integers(1, 5000, 400)), "ones": [1] * 3000}


def check_chunking(be: Backend, plans=None):
    """three channels, the last one clipping: every chunking gives the bytes and clip counts of the single push"""
    names, gains = ["lr80", "cnr40", "l1k"], [1.0, 1.0, 4.0]
    x = stack(names)
    D = be.demod(3, gains=gains)
    ref, ref_clips = run(be, D, x, [])
    assert ref_clips[2, 0] > 0 and ref.shape[1] == 6080
    for c, name in enumerate(names):
        compare(ref[c], ref_clips[c], name, gains[c])
    all_plans = chunk_plans(fa.N)
    for plan in plans or all_plans:
        D.reset()
        out, clips = run(be, D, x, all_plans[plan])
        assert out.tobytes() == ref.tobytes(), plan
        assert np.array_equal(clips, ref_clips), plan
    D.close()


def check_reset_overflow_bad_arguments(be: Backend):
    x = stack(["l1k", "mono"])
    n = fa.N
    D = be.demod(2)
    first, c1 = run(be, D, x, [33333])
    lv1 = D.pilot()
    D.reset()
    lv0 = D.pilot()
    assert not lv0[0].any() and not lv0[1].any() and not D.clip_counts().any()
    assert D.outputs_for(n) == first.shape[1]
    # EOVERFLOW leaves the object untouched
    keep_in, p_in = be.upload(x)
    keep_out, p_out = be.zeros((2, first.shape[1], 2))
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.process(p_in, 2 * n, n, p_out, 2 * first.shape[1], first.shape[1] - 1)
    assert ei.value.code == eng.EOVERFLOW
    assert D.outputs_for(n) == first.shape[1]
    bad = [(p_in, 2 * n, -1, p_out, 2 * first.shape[1], first.shape[1]),          # negative count
           (0, 2 * n, n, p_out, 2 * first.shape[1], first.shape[1]),              # null input
           (p_in + 2, 2 * n, n - 1, p_out, 2 * first.shape[1], first.shape[1]),   # input not on a sample boundary
           (p_in, 2 * n + 1, n, p_out, 2 * first.shape[1], first.shape[1]),       # odd stride
           (p_in, 2 * n - 2, n, p_out, 2 * first.shape[1], first.shape[1]),       # channels overlap
           (p_in, 2 * n, n, 0, 2 * first.shape[1], first.shape[1]),               # null output
           (p_in, 2 * n, n, p_out, first.shape[1], first.shape[1]),               # output stride shorter than the capacity
           (p_in, 2 * n, n, p_out, 2 * first.shape[1], -1)]
    for args in bad:
        with pytest.raises(eng.Nrsc5HipError) as ei:
            D.process(*args)
        assert ei.value.code == eng.EINVAL, args
    with pytest.raises(eng.Nrsc5HipError) as ei:
        D.outputs_for(-1)
    assert "negative" in str(ei.value)
    second, c2 = run(be, D, x, [])                                                 # ... and a reset object equals a fresh one
    assert second.tobytes() == first.tobytes() and np.array_equal(c1, c2)
    lv2 = D.pilot()
    assert np.array_equal(lv1[0], lv2[0]) and np.array_equal(lv1[1], lv2[1])
    D.close()
    for kw in (dict(nchan=0), dict(nchan=513), dict(nchan=1, deemphasis_us=60.0), dict(nchan=1, pilot_min=-0.1), dict(nchan=1, pilot_min=float("nan")),
               dict(nchan=2, gains=[1.0, float("inf")])):
        with pytest.raises(eng.Nrsc5HipError) as ei:
            be.demod(**kw)
        assert ei.value.code == eng.EINVAL, kw


# -------------------------------------------------------------------------------------------------------------------- edge cases
def check_edges(be: Backend):
    names = ["mono", "zero", "pilot02", "pilot04", "l1k"]
    D = be.demod(len(names))
    got, clips = run(be, D, stack(names), [40000, 40001])
    level, stereo = D.pilot()
    D.close()
    for c, name in enumerate(names):
        compare(got[c], clips[c], name)
        _, _, info = fa.reference(name)
        assert stereo[c] == info["stereo"][-1] and abs(level[c] - info["level"][-1]) < 1e-5, (name, level[c], info["level"][-1])
    assert np.array_equal(got[0][:, 0], got[0][:, 1]) and not stereo[0] and np.abs(got[0]).max() > 5000      # mono host: L == R on every sample
    assert not got[1].any() and not stereo[1] and level[1] == 0.0                                            # silence in, silence out
    assert not stereo[2] and abs(level[2] - 0.02) < 0.002 and np.array_equal(got[2][:, 0], got[2][:, 1])     # pilot under pilot_min
    assert stereo[3] and abs(level[3] - 0.04) < 0.002 and not np.array_equal(got[3][:, 0], got[3][:, 1])     # ... and over it
    assert stereo[4] and abs(level[4] - 0.1) < 0.002
    # pilot_min is honoured: the 0.04 pilot is mono for a demodulator that asks for 0.05
    D = be.demod(1, pilot_min=0.05)
    got, _ = run(be, D, stack(["pilot04"]), [])
    assert not D.pilot()[1][0] and np.array_equal(got[0][:, 0], got[0][:, 1])
    D.close()


# ---------------------------------------------------------------------------------------------------------------- physical checks
# name -> (tone Hz, channel it is on, programme level, least separation dB)
PHYSICAL = {"l1k": (1000.0, 0, 0.3, 40.0), "ppm_plus": (1000.0, 0, 0.3, 40.0), "ppm_minus": (1000.0, 0, 0.3, 40.0), "cnr40": (1000.0, 0, 0.3, 40.0),
            "r10k": (10000.0, 1, 0.1, 30.0)}


def physical(pcm: np.ndarray, name: str):
    """-> (tone level relative to 0.9 a 32767 in dB, separation in dB); asserts the bounds"""
    f, on, a, sep_min = PHYSICAL[name]
    amp_db = 20 * np.log10(fm.tone(pcm[:, on], f, fm.SETTLE) / (0.9 * a * 32767))
    sep = fm.separation_db(pcm, f, on)
    assert abs(amp_db) <= 0.1, (name, amp_db)
    assert sep >= sep_min, (name, sep)
    return float(amp_db), sep


def check_physical(be: Backend):
    names = list(PHYSICAL)
    D = be.demod(len(names))
    got, _ = run(be, D, stack(names), [])
    D.close()
    for c, name in enumerate(names):
        m_amp, m_sep = physical(fa.reference(name)[0], name)
        l_amp, l_sep = physical(got[c], name)
        print(f"{name}: tone {l_amp:+.3f} dB (model {m_amp:+.3f} dB), separation {l_sep:.1f} dB (model {m_sep:.1f} dB)")
        assert abs(l_amp - m_amp) <= 1.0 and abs(l_sep - m_sep) <= 1.0, (name, l_amp, m_amp, l_sep, m_sep)


def shares_report(be: Backend) -> list:
    """the lines of profiles/wideband_analog_cases.txt: every input's share of samples that differ from the float64 model"""
    lines = []
    for name in fa.CASES:
        share = check_audio_case(be, name)
        ref = fa.reference(name)
        lines.append(f"{name:10s} differing {100 * share:.4f} %  float32 model {100 * ref[2]['share32']:.4f} %  rms {np.sqrt(np.mean(ref[0].astype(np.float64) ** 2)):7.0f} LSB")
    return lines
