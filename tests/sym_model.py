"""The FM symbol transform of one block -- what k_mixfft / k_mixfft8 compute (timing pick, Q15 -> float conjugated, oscillator mix, raised-cosine cyclic-prefix fold,
FFT-2048, fftshift, live-bin cut) -- in float64 numpy, written from the definition in the reference (acquire.c:160-168, 237-254; defines.h:106-123; sync.c:785-789)
and not from the kernel: what nrsc5hip_stage_symbols is checked against (tests/sym_checks.py).

  sample j of symbol sym   x = conj(q15[a00 + sym * 2160 + j]) / 32767                         (cq15_to_cf_conj)
  oscillator               p = exp(i (theta + (sym * 2160 + j) dtheta)) (1 + growth)^j            (phase *= phase_increment per sample, renormalised per symbol),
                           or the caller's table entry [sym][j] in exact mode
  shape and fold           fftin[j] = shape[j] p x  (j < 2048),   fftin[j - 2048] += shape[j] p x  (j >= 2048)
  transform                np.fft.fft in complex128, fftshift, bins 478 .. 744 and 1304 .. 1570

shape is acquire.c:322-331 in float64: sin(a) for j < 112, 1 up to 2047, cos(a') behind, with a = pi / 2 * j / 112 and a' = pi / 2 * (j - 2048) / 112 rounded to
float32 as sinf / cosf receive them.  The engine does not expose the table it uploads (DevTables::shape); it is built in csrc/engine.hip (build_tables) from the same
three lines with the host's sinf / cosf, i.e. within an ulp of shape32() below -- 6e-8 of a sample, far inside the bounds of tests/sym_args.py.

reference32() is the same block in the reference's own ARITHMETIC -- float32, unfused: the two divisions of cq15_to_cf_conj, the four products and two sums of the
complex multiplication, the real-by-complex shape products, the fold's addition, and the oracle's float FFT -- on given float32 phasors: the yardstick the
transform's float32 error is measured with (tests/sym_args.py: SYM_ERR_MEASURED), never an expected value."""
import numpy as np

FFT_N, CP_N, SYM_N, NSYM = 2048, 112, 2160, 32
LB0, UB0, LIVE_HALF, LIVE_N = 478, 1304, 267, 534
LIVE_BINS = np.concatenate([np.arange(LB0, LB0 + LIVE_HALF), np.arange(UB0, UB0 + LIVE_HALF)])
LIVE_BINS.setflags(write=False)
F32 = np.float32


def shape64():
    """acquire.c:322-331: sinf / cosf take a FLOAT, so the double argument is rounded to float32 first (near pi / 2 that rounding is 4e-6 of the cosine); the sine and
    cosine of that float in float64"""
    j = np.arange(SYM_N, dtype=np.float64)
    s = np.ones(SYM_N)
    s[:CP_N] = np.sin((np.pi / 2 * j[:CP_N] / CP_N).astype(F32).astype(np.float64))
    s[FFT_N:] = np.cos((np.pi / 2 * (j[FFT_N:] - FFT_N) / CP_N).astype(F32).astype(np.float64))
    return s


def shape32():
    return shape64().astype(F32)


def slot_of(b):
    """slot of (shifted) FFT bin b in a row of 534, or -1 for a bin the cut drops"""
    if LB0 <= b < LB0 + LIVE_HALF:
        return b - LB0
    if UB0 <= b < UB0 + LIVE_HALF:
        return LIVE_HALF + b - UB0
    return -1


def phasors(theta, dtheta, growth):
    """the closed-form oscillator of one block: complex128 [32, 2160]"""
    j = np.arange(SYM_N, dtype=np.float64)[None, :]
    sym = np.arange(NSYM, dtype=np.float64)[:, None]
    return np.exp(1j * (theta + (sym * SYM_N + j) * dtheta)) * (1.0 + growth) ** j


def table_phasors(tab):
    """an oscillator table float32 [32, 2160, 2] as complex128 [32, 2160]"""
    t = np.asarray(tab, dtype=np.float64).reshape(NSYM, SYM_N, 2)
    return t[..., 0] + 1j * t[..., 1]


def block_samples(q15, a00):
    """the 32 x 2160 Q15 samples of the block that starts at a00: int64 [32, 2160, 2]"""
    q = np.asarray(q15).reshape(-1, 2)[a00:a00 + NSYM * SYM_N].astype(np.int64)
    assert q.shape[0] == NSYM * SYM_N
    return q.reshape(NSYM, SYM_N, 2)


def transform(q15, a00, ph):
    """-> (bins complex128 [32, 534], weight float64 [32]): the model, and sum_j shape[j] |sample_j| / 32767 per symbol -- what an error of the oscillator's
    phasor is multiplied by at most on its way into any bin"""
    q = block_samples(q15, a00)
    x = (q[..., 0] - 1j * q[..., 1]) / 32767.0
    sh = shape64()
    m = sh[None, :] * ph * x
    fftin = m[:, :FFT_N].copy()
    fftin[:, :CP_N] += m[:, FFT_N:]
    out = np.fft.fftshift(np.fft.fft(fftin, axis=1), axes=1)
    return out[:, LIVE_BINS], (sh[None, :] * np.abs(x)).sum(axis=1)


def reference32(oracle, q15, a00, ph):
    """the block in the reference's float32 arithmetic on the phasors ph rounded to float32 -> complex128 [32, 534] (of float32 values)"""
    q = block_samples(q15, a00)
    c = q[..., 0].astype(F32) / F32(32767.0)
    d = q[..., 1].astype(F32) / F32(-32767.0)
    a, b = ph.real.astype(F32), ph.imag.astype(F32)
    re, im = a * c - b * d, a * d + b * c                       # (numpy rounds every float32 product and sum: no contraction)
    assert re.dtype == F32 and im.dtype == F32
    sh = shape32()
    fre, fim = re[:, :FFT_N].copy(), im[:, :FFT_N].copy()
    fre[:, :CP_N] = sh[:CP_N] * re[:, :CP_N]; fim[:, :CP_N] = sh[:CP_N] * im[:, :CP_N]
    fre[:, :CP_N] += sh[FFT_N:] * re[:, FFT_N:]; fim[:, :CP_N] += sh[FFT_N:] * im[:, FFT_N:]
    out = np.empty((NSYM, LIVE_N), dtype=np.complex128)
    for s in range(NSYM):
        x = np.empty(FFT_N, dtype=np.complex64)
        x.real, x.imag = fre[s], fim[s]
        out[s] = np.fft.fftshift(oracle.fft(x))[LIVE_BINS]
    return out
