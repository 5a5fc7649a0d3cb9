"""Float64 restatement of the analog FM demodulator's definition (include/nrsc5hip.h "analog FM audio"), in numpy: what
nrsc5hip_fm_* is checked against.  dtype=np.float32 runs the same sums in float32: the reference's own estimate of how far a float32
implementation may sit from the float64 one."""
import numpy as np

FS = 744187.5
FS1 = FS / 2                                   # 372 093.75 S/s behind the channel filter
AUDIO_RATE = 44100                             # FS1 * 16 / 135, exactly
PHASES, T_NUM = 16, 135                        # output k at t_k = 135 k / 16 FS1 samples
BLOCK, BLOCK_OUT = 540, 64                     # one pilot block: 540 FS1 samples = 64 audio outputs = 1080 input samples
PILOT_NUM, PILOT_DEN = 608, 11907              # 19 kHz = 608 / 11907 cycles per FS1 sample
W = 16                                         # pilot smoothing: 2 W + 1 blocks
LATENCY_IN = 2 * BLOCK * (W + 1) - 1           # audio block j exists once LATENCY_IN + 1080 j input samples have arrived
TA = 112                                       # channel filter taps
PASS_A, STOP_A, ATT_A = 95e3, 129361.0, 80.0   # channel filter: passband edge, first primary-main carrier, Kaiser design target
PASS_B, STOP_B, ATT_B = 15e3, 19e3, 66.0       # audio prototype at 16 FS1
DEV_SCALE = FS1 / (2 * np.pi * 75000.0)        # +-75 kHz -> +-1
EQ_F = (28000.0, 48000.0)                      # the droop equaliser is exact at these two frequencies


def kaiser_lowpass(taps: int, fc: float, att_db: float) -> np.ndarray:
    """fc in cycles per sample; symmetric about (taps - 1) / 2"""
    beta = 0.1102 * (att_db - 8.7)
    tau = np.arange(taps, dtype=np.float64) - (taps - 1) / 2
    u = 2 * tau / (taps - 1)
    w = np.i0(beta * np.sqrt(np.clip(1 - u * u, 0, None))) / np.i0(beta)
    return 2 * fc * np.sinc(2 * fc * tau) * w


def kaiser_taps(att_db: float, dw: float) -> int:
    return int(np.ceil((att_db - 7.95) / (2.285 * dw))) + 1


def design_ha() -> np.ndarray:
    h = kaiser_lowpass(TA, 0.5 * (PASS_A + STOP_A) / FS, ATT_A)
    return h / h.sum()


def design_eq():
    """3-tap symmetric FIR (a, b, a) whose response b + 2 a cos(w) equals 1 / sinc(f / FS1) at EQ_F"""
    r = [1.0 / np.sinc(f / FS1) for f in EQ_F]
    c = [np.cos(2 * np.pi * f / FS1) for f in EQ_F]
    a = (r[0] - r[1]) / (2 * (c[0] - c[1]))
    return a, r[0] - 2 * a * c[0]


def design_audio(deemphasis_us: float) -> np.ndarray:
    """the prototype at 16 FS1 (virtual index v), DC gain 16; -> float64 [PHASES][TB], row p column j = g[16 j + p]"""
    fv = PHASES * FS1
    nk = kaiser_taps(ATT_B, 2 * np.pi * (STOP_B - PASS_B) / fv)
    g = kaiser_lowpass(nk, 0.5 * (PASS_B + STOP_B) / fv, ATT_B)
    if deemphasis_us > 0:
        tf = deemphasis_us * 1e-6 * fv
        ne = int(np.ceil(30 * np.log(2.0) * tf))                # exp(-v / tf) < 2^-30 from here on
        e = np.exp(-np.arange(ne, dtype=np.float64) / tf)
        e[0] = 0.5                                               # the step at t = 0 sampled at its mid value (trapezoidal rule)
        g = np.convolve(g, e)
    g = g * (PHASES / g.sum())
    tb = (g.size + PHASES - 1) // PHASES
    full = np.zeros(tb * PHASES)
    full[:g.size] = g
    return np.ascontiguousarray(full.reshape(tb, PHASES).T)


def pilot_window() -> np.ndarray:
    w = np.arange(-W, W + 1, dtype=np.float64)
    return 0.5 * (1 + np.cos(np.pi * w / (W + 1)))


def outputs_total(n_in: int) -> int:
    return BLOCK_OUT * max(0, ((n_in + 1) // 2) // BLOCK - W)


def front(x: np.ndarray, ha: np.ndarray, dtype=np.float64):
    """x int16 [n, 2] -> d [ceil(n / 2)], block sums p [complete blocks] (complex)"""
    ct = np.complex128 if dtype == np.float64 else np.complex64
    xc = (x[:, 0].astype(dtype) + 1j * x[:, 1].astype(dtype)).astype(ct)
    m1 = (x.shape[0] + 1) // 2
    z = np.convolve(xc, ha.astype(dtype))[0:2 * m1:2].astype(ct)
    zp = np.concatenate([np.zeros(1, ct), z[:-1]])
    pr = (z * np.conj(zp)).astype(ct)
    re, im = pr.real.astype(dtype), pr.imag.astype(dtype)
    d = (np.arctan2(im, re).astype(dtype) * dtype(DEV_SCALE)).astype(dtype)
    d[(re == 0) & (im == 0)] = 0
    if d.size:
        d[0] = 0
    nb = m1 // BLOCK
    idx = (PILOT_NUM * np.arange(nb * BLOCK, dtype=np.int64)) % PILOT_DEN
    ang = 2 * np.pi * idx / PILOT_DEN
    e = (np.cos(ang).astype(dtype) - 1j * np.sin(ang).astype(dtype)).astype(ct)
    p = (d[:nb * BLOCK] * e).reshape(nb, BLOCK).sum(axis=1).astype(ct)
    return d, p


def model(x: np.ndarray, ha: np.ndarray, tab: np.ndarray, deemphasis_us: float = 75.0, gain: float = 1.0, pilot_min: float = 0.03,
          dtype=np.float64):
    """one channel.  x int16 [n, 2]; ha, tab: the tables as the library stores them (float32).
    -> pcm int16 [n_out, 2], clips [2], info {"d", "psum", "level" [blocks], "stereo" [blocks], "v": unrounded [n_out, 2]}"""
    ha = np.asarray(ha, dtype=np.float32).astype(dtype)
    tab = np.asarray(tab, dtype=np.float32).astype(dtype)
    tb = tab.shape[1]
    d, p = front(x, ha, dtype)
    nblk = max(0, p.size - W)
    win = pilot_window()
    wsum = win.sum()
    aq, bq = (dtype(v) for v in (np.float32(design_eq()[0]), np.float32(design_eq()[1])))
    ppad = np.concatenate([np.zeros(W, p.dtype), p])
    dpad = np.concatenate([np.zeros(tb + 2, dtype), d, np.zeros(2, dtype)])       # dpad[m + tb + 2] = d[m]
    off = tb + 2
    scale = dtype(np.float32(32767.0 * gain))
    v = np.zeros((nblk * BLOCK_OUT, 2), dtype)
    level, stereo = np.zeros(nblk), np.zeros(nblk, bool)
    jj = np.arange(tb, dtype=np.int64)
    winf = win.astype(np.float32).astype(dtype)
    for j in range(nblk):
        ph = (ppad[j:j + 2 * W + 1] * winf).sum()
        mag = dtype(np.hypot(dtype(ph.real), dtype(ph.imag)))
        a = dtype(2) * mag / dtype(BLOCK) / dtype(np.float32(wsum))
        level[j], stereo[j] = a, a >= dtype(np.float32(pilot_min))
        k = np.arange(BLOCK_OUT * j, BLOCK_OUT * (j + 1), dtype=np.int64)
        ik, pk = (T_NUM * k) >> 4, (T_NUM * k) & 15
        gat = (ik[:, None] - jj[None, :]) + off
        rows = tab[pk]
        s = (rows * dpad[gat]).sum(axis=1)
        dl = np.zeros(BLOCK_OUT, dtype)
        if stereo[j]:
            ur, ui = dtype(ph.real) / mag, dtype(ph.imag) / mag
            c2, s2 = -(ur * ur - ui * ui), -(dtype(2) * ur * ui)
            m = np.arange(BLOCK * j - tb, BLOCK * j + BLOCK, dtype=np.int64)       # covers every index the block's outputs read
            ang = 2 * np.pi * ((2 * PILOT_NUM * m) % PILOT_DEN) / PILOT_DEN
            sub = np.sin(ang).astype(dtype) * c2 + np.cos(ang).astype(dtype) * s2
            mm = m + off
            span = dtype(2) * (aq * dpad[mm - 1] + bq * dpad[mm] + aq * dpad[mm + 1]) * sub
            span[m < 0] = 0
            dl = (rows * span[gat - (BLOCK * j - tb + off)]).sum(axis=1)
        v[k, 0], v[k, 1] = (s + dl) * scale, (s - dl) * scale
    r = np.rint(v.astype(np.float64))
    clips = np.array([np.sum((r[:, c] > 32767) | (r[:, c] < -32768)) for c in (0, 1)], dtype=np.int64)
    pcm = np.clip(r, -32768, 32767).astype(np.int16)
    return pcm, clips, {"d": d, "psum": p, "level": level, "stereo": stereo, "v": v}


def response_db(h: np.ndarray, freqs: np.ndarray, fs: float) -> np.ndarray:
    """|H(f)| / |H(0)| in dB"""
    n = np.arange(h.size)
    out = []
    for b in range(0, freqs.size, 256):
        out.append(np.abs(np.exp(-2j * np.pi * np.outer(freqs[b:b + 256], n) / fs) @ h))
    return 20 * np.log10(np.maximum(np.concatenate(out) / abs(h.sum()), 1e-30))


def prototype(tab: np.ndarray) -> np.ndarray:
    """[PHASES][TB] -> the prototype at 16 FS1"""
    return np.ascontiguousarray(np.asarray(tab, dtype=np.float64).T).reshape(-1)


def tone(pcm: np.ndarray, f: float, skip: int) -> float:
    """amplitude of the tone at f Hz in pcm[skip:] (one channel), by a Hann-windowed projection"""
    y = np.asarray(pcm[skip:], dtype=np.float64)
    n = y.size
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n)
    return float(2 * abs(np.sum(w * y * np.exp(-2j * np.pi * f * np.arange(n) / AUDIO_RATE))) / w.sum())


SETTLE = BLOCK_OUT * (2 * W + 4)               # audio outputs behind which the pilot window no longer reaches in front of the stream


def separation_db(pcm: np.ndarray, f: float, on: int = 0) -> float:
    """level of the tone at f in channel `on` over its level in the other channel, dB"""
    a, b = tone(pcm[:, on], f, SETTLE), tone(pcm[:, 1 - on], f, SETTLE)
    return float(20 * np.log10(a / max(b, 1e-9)))
