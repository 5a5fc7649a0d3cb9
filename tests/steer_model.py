"""Float64 restatement of reception steering (include/nrsc5hip.h "reception steering"), in numpy: what nrsc5hip_fm_steer* and the
steered audio are checked against.  It reuses tests/fm_model.py (front end, pilot, tables) and tests/carrier_model.py (envelope, block triples,
the window and the butterfly).  dtype=np.float32 runs the front end, the ramps and the audio sums in float32 (the block triples and q stay double, as
the definition has them): the reference's own estimate of how far a float32 implementation may sit from the float64 one."""
import numpy as np

from tests import carrier_model as cm, fm_model as fm

BLOCK, BLOCK_OUT, W = fm.BLOCK, fm.BLOCK_OUT, fm.W
BLEND, HIGHCUT, MUTE, ALL = 1, 2, 4, 7
DEFAULTS = dict(blend_db=(18.0, 30.0), highcut_db=(10.0, 20.0), mute_db=(2.0, 8.0), mute_floor_db=-20.0, controls=ALL)
PASS_N, STOP_N = 4e3, 8e3                      # the narrow prototype's edges


def config(**kw) -> dict:
    cfg = dict(DEFAULTS)
    cfg.update({k: v for k, v in kw.items() if v is not None})
    return cfg


def q_of_db(db: float) -> float:
    """a threshold in dB CNR (in the channel filter's bandwidth) as a value of q = (S / P)^2"""
    rho = 10.0 ** (db / 10.0)
    u = rho / (1.0 + rho)
    return u * u


def ramp(db) -> tuple:
    """[lo_db, hi_db] -> (q_lo, inv) as stored: float32"""
    q_lo, q_hi = q_of_db(db[0]), q_of_db(db[1])
    return np.float32(q_lo), np.float32(1.0 / (q_hi - q_lo))


def design_narrow(deemphasis_us: float) -> np.ndarray:
    """the narrow prototype, built as fm_model.design_audio builds the wide one -> float64 [PHASES][TB]"""
    fv = fm.PHASES * fm.FS1
    nk = fm.kaiser_taps(fm.ATT_B, 2 * np.pi * (STOP_N - PASS_N) / fv)
    g = fm.kaiser_lowpass(nk, 0.5 * (PASS_N + STOP_N) / fv, fm.ATT_B)
    if deemphasis_us > 0:
        tf = deemphasis_us * 1e-6 * fv
        ne = int(np.ceil(30 * np.log(2.0) * tf))
        e = np.exp(-np.arange(ne, dtype=np.float64) / tf)
        e[0] = 0.5
        g = np.convolve(g, e)
    g = g * (fm.PHASES / g.sum())
    tb = (g.size + fm.PHASES - 1) // fm.PHASES
    full = np.zeros(tb * fm.PHASES)
    full[:g.size] = g
    return np.ascontiguousarray(full.reshape(tb, fm.PHASES).T)


def quality(t: np.ndarray) -> np.ndarray:
    """block triples t [blocks][3] -> q float64 [audio blocks]: the windowed sums in the report's order (lane w + W holds term w, the butterfly),
    c_j the window's weight over the blocks that exist"""
    win = cm.window32()
    nblk = max(0, t.shape[0] - W)
    q = np.zeros(nblk)
    for j in range(nblk):
        l2, l4, lc = np.zeros(64), np.zeros(64), np.zeros(64)
        for lane in range(2 * W + 1):
            jb = j + lane - W
            if jb >= 0:
                l2[lane], l4[lane], lc[lane] = t[jb, 0] * win[lane], t[jb, 1] * win[lane], win[lane]
        w2, w4, c = cm.butterfly(l2), cm.butterfly(l4), cm.butterfly(lc)
        if w2 > 0:
            kappa = w4 * (540.0 * c) / (w2 * w2)
            q[j] = min(1.0, max(0.0, 2.0 - kappa))
    return q


def factors(q: np.ndarray, cfg: dict, dtype=np.float64) -> np.ndarray:
    """q [blocks] -> [blocks][4]: (q, b, h, g) in dtype: in float32 q is rounded in front of the ramps, as the definition has it, in float64 it is not"""
    qf = np.asarray(q, dtype=np.float64).astype(dtype)
    out = np.ones((qf.size, 4), dtype)
    out[:, 0] = qf
    one, zero = dtype(1), dtype(0)
    for col, key, bit in ((1, "blend_db", BLEND), (2, "highcut_db", HIGHCUT), (3, "mute_db", MUTE)):
        if not cfg["controls"] & bit:
            continue
        lo, inv = (dtype(v) for v in ramp(cfg[key]))
        f = np.minimum(one, np.maximum(zero, ((qf - lo).astype(dtype) * inv).astype(dtype)))
        if bit == MUTE:
            floor = dtype(np.float32(10.0 ** (cfg["mute_floor_db"] / 20.0)))
            f = (f.astype(np.float64) * np.float64(dtype(one - floor)) + np.float64(floor)).astype(dtype)      # fma(f, 1 - floor, floor)
        out[:, col] = f
    return out


def model(x: np.ndarray, ha: np.ndarray, tab: np.ndarray, tab_n: np.ndarray, cfg: dict, gain: float = 1.0, pilot_min: float = 0.03,
          given: np.ndarray | None = None, dtype=np.float64):
    """one channel, steered.  x int16 [n, 2]; ha, tab, tab_n: the tables as the library stores them (float32); given: (q, b, h, g) per audio block to
    use in place of the model's own (the device's, for a check of the mixing alone).
    -> pcm int16 [n_out, 2], clips [2], info {"t", "q", "factors" [blocks][4], "stereo", "v": unrounded [n_out, 2]}"""
    ha = np.asarray(ha, dtype=np.float32)
    tab, tab_n = (np.asarray(v, dtype=np.float32).astype(dtype) for v in (tab, tab_n))
    tb = tab.shape[1]
    d, p = fm.front(x, ha.astype(dtype), dtype)
    _, _, t = cm.front(x, ha, dtype)
    nblk = max(0, p.size - W)
    q = quality(t)
    fac = factors(q, cfg, dtype) if given is None else np.asarray(given, dtype=np.float32).astype(dtype)
    assert fac.shape == (nblk, 4)
    win = fm.pilot_window()
    wsum = win.sum()
    aq, bq = (dtype(v) for v in (np.float32(fm.design_eq()[0]), np.float32(fm.design_eq()[1])))
    ppad = np.concatenate([np.zeros(W, p.dtype), p])
    dpad = np.concatenate([np.zeros(tb + 2, dtype), d, np.zeros(2, dtype)])       # dpad[m + tb + 2] = d[m]
    off = tb + 2
    scale = dtype(np.float32(32767.0 * gain))
    v = np.zeros((nblk * BLOCK_OUT, 2), dtype)
    stereo = np.zeros(nblk, bool)
    jj = np.arange(tb, dtype=np.int64)
    winf = win.astype(np.float32).astype(dtype)
    frac = (np.arange(1, BLOCK_OUT + 1).astype(dtype) / dtype(64)).astype(dtype)
    one = dtype(1)
    for j in range(nblk):
        ph = (ppad[j:j + 2 * W + 1] * winf).sum()
        mag = dtype(np.hypot(dtype(ph.real), dtype(ph.imag)))
        a = dtype(2) * mag / dtype(BLOCK) / dtype(np.float32(wsum))
        stereo[j] = a >= dtype(np.float32(pilot_min))
        k = np.arange(BLOCK_OUT * j, BLOCK_OUT * (j + 1), dtype=np.int64)
        ik, pk = (fm.T_NUM * k) >> 4, (fm.T_NUM * k) & 15
        gat = (ik[:, None] - jj[None, :]) + off
        src = dpad[gat]
        sw, sn = (tab[pk] * src).sum(axis=1).astype(dtype), (tab_n[pk] * src).sum(axis=1).astype(dtype)
        dw, dn = np.zeros(BLOCK_OUT, dtype), np.zeros(BLOCK_OUT, dtype)
        if stereo[j]:
            ur, ui = dtype(ph.real) / mag, dtype(ph.imag) / mag
            c2, s2 = -(ur * ur - ui * ui), -(dtype(2) * ur * ui)
            m = np.arange(BLOCK * j - tb, BLOCK * j + BLOCK, dtype=np.int64)
            ang = 2 * np.pi * ((2 * fm.PILOT_NUM * m) % fm.PILOT_DEN) / fm.PILOT_DEN
            sub = np.sin(ang).astype(dtype) * c2 + np.cos(ang).astype(dtype) * s2
            mm = m + off
            span = dtype(2) * (aq * dpad[mm - 1] + bq * dpad[mm] + aq * dpad[mm + 1]) * sub
            span[m < 0] = 0
            dsrc = span[gat - (BLOCK * j - tb + off)]
            dw, dn = (tab[pk] * dsrc).sum(axis=1).astype(dtype), (tab_n[pk] * dsrc).sum(axis=1).astype(dtype)
        c0, c1 = fac[max(j - 1, 0), 1:], fac[j, 1:]
        b, h, g = (((c1[i] - c0[i]) * frac + c0[i]).astype(dtype) for i in range(3))
        sp = (h * sw + ((one - h) * sn).astype(dtype)).astype(dtype)
        dp = (h * dw + ((one - h) * dn).astype(dtype)).astype(dtype)
        bd = (b * dp).astype(dtype)
        v[k, 0], v[k, 1] = ((sp + bd) * g).astype(dtype) * scale, ((sp - bd) * g).astype(dtype) * scale
    r = np.rint(v.astype(np.float64))
    clips = np.array([np.sum((r[:, c] > 32767) | (r[:, c] < -32768)) for c in (0, 1)], dtype=np.int64)
    pcm = np.clip(r, -32768, 32767).astype(np.int16)
    return pcm, clips, {"t": t, "q": q, "factors": fac, "stereo": stereo, "v": v}
