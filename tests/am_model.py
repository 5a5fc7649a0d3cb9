"""Float64 restatement of ONE block of the AM receiver -- what k_am_block (nrsc5_amd/csrc/k_am.hip) restates of acquire.c:110-262 (AM geometry),
sync.c:209-252 / 612-767 and decode.c:474-505 -- in plain numpy, every step once: what nrsc5hip_stage_am_block is checked against (tests/am_checks.py), pinned
itself to the oracle's log of whole captures (tests/test_am_block_stage_cpu.py).

Arithmetic is float64 / complex128 (np.fft).  Rounded to float32 is only what the reference DEFINES as a float and carries on with: the pulse-shape table, the state
words prev_angle / angle, and the oscillator's increment -- phase_increment is a float complex (acquire.c:168, 232), so the step the whole block turns by is the angle
of that ROUNDED pair (6e-8 rad per sample = 5e-4 rad over a block for another rounding).  The oscillator itself is closed form: theta + dtheta * sample.

Besides the block's results block() returns how far every decision sits from flipping: per sliced cell the distance to the nearest slicer boundary in grid units,
for the timing estimate the distance of `se` from a half-integer, for the CFO arg-max the ratio of the two largest sums, and how often half_turn_diff wrapped."""
import numpy as np

FFT, CP, SYM, NSYM, WIN, PW = 256, 14, 270, 32, 8910, 25
NONE, COARSE, FINE = 0, 1, 2
MA3 = 2
FS = 46511.71875
REC_PROCESSED, REC_TO_COARSE, REC_TO_FINE, REC_PIDS = 1, 2, 4, 16
CARE23, VAL23 = 0x60427f, 0x600226                               # positions 0-6, 9, 14, 21, 22 of the reference sequence; ones at 1, 2, 5, 9, 21, 22 (sync.c:211-213)
PARITY_GROUPS = ((7, 8), (10, 11, 12, 13), (15, 16, 17, 18, 19, 20), tuple(range(23, 32)))
STATE_DEFAULTS = dict(sync_state=NONE, samperr=0, cfo=0, psmi=1, bc=0, cfo_wait=0, prev_angle=0.0, angle=0.0, theta=0.0, coarse_samperr=0, coarse_re=0.0, coarse_im=0.0,
                      keep_extra=0, offset_history=0, rdbi=-1, pli=-1, hppi=-1, aabi=-1, am_diversity_wait=4, am_errors=0, fine_epoch=0, active=0, nblocks=0, rd=0)
PIDS_IL_POS = (0, 1, 12, 13, 6, 5, 18, 17, 11, 7, 23, 19)        # decode.c:63-64
PIDS_IU_POS = (2, 4, 14, 16, 3, 8, 15, 20, 9, 10, 21, 22)
ACQ_TAPS = (-0.00038464731187559664, -0.00021618751634377986, 0.0026779419276863337, -0.00029802651260979474, -0.0012626448879018426, -0.0013182522961869836,
            -0.012252614833414555, 0.015980124473571777, 0.037112727761268616, -0.05451361835002899, -0.05804193392395973, 0.11320608854293823,
            0.055298302322626114, -0.16878043115139008, -0.022917453199625015, 0.19178225100040436)         # acquire.c:63-96, first half (symmetric about tap 15; tap 31 = 0)
_SLICE8 = np.array([0, 4, 6, 2, 3, 7, 5, 1], dtype=np.uint8)     # sync.c:49-67: the code of the interval between the boundaries -3 .. 3
_SLICE4 = np.array([0, 2, 3, 1], dtype=np.uint8)                 # sync.c:37-47: boundaries -1, 0, 1
_B8, _B4 = np.arange(-3.0, 4.0), np.arange(-1.0, 2.0)
f32 = np.float32


def pulse_shape():
    """acquire.c:333-342, the float table"""
    i = np.arange(SYM, dtype=np.float64)
    s = np.ones(SYM)
    s[:CP] = np.sin(np.pi / 2 * i[:CP] / CP)
    s[FFT:] = np.cos(np.pi / 2 * (i[FFT:] - FFT) / CP)
    return s.astype(f32).astype(np.float64)


SHAPE = pulse_shape()


def q15_to_c(x):
    x = np.asarray(x, dtype=np.float64)
    return (x[..., 0] + 1j * x[..., 1]) / 32767.0               # cq15_to_cf, defines.h:106


# ---- coarse acquisition (acquire.c:120-151) ------------------------------------------------------------------------------------------------------
def acquire(win, hist):
    """band-select FIR in the reference's int16 arithmetic (exact), cyclic-prefix correlation in float64 -> (samperr, peak, ratio of the two largest |v|^2)"""
    q = (np.array(ACQ_TAPS, dtype=f32) * f32(32767.0)).astype(np.int16).astype(np.int64)        # q[k] = tap k; the kernel's acq_q15[i] = tap 31 - i = tap i - 1
    w = np.concatenate([np.asarray(hist, dtype=np.int64), np.asarray(win, dtype=np.int64)])     # a[i] = w[t + i]
    acc = np.zeros((WIN, 2), dtype=np.int64)
    for i in range(1, 16):
        acc += ((w[i:i + WIN] + w[32 - i:32 - i + WIN]) * q[i - 1]) >> 15
    acc += (w[16:16 + WIN] * q[15]) >> 15
    filt = ((acc + 32768) % 65536 - 32768)                                                    # the int16 accumulator wraps; sums of wrapped terms wrap alike
    b = q15_to_c(filt)
    i = np.arange(SYM)[:, None] + SYM * np.arange(NSYM)[None, :]
    sums = (b[i] * np.conj(b[i + FFT])).sum(axis=1)
    k = (np.arange(SYM)[:, None] + np.arange(CP)[None, :]) % SYM
    v = (sums[k] * (SHAPE[:CP] * SHAPE[FFT:])[None, :]).sum(axis=1)
    mag = np.abs(v) ** 2
    best = int(np.argmax(mag))                                                                  # first maximum in index order
    rest = np.delete(mag, best)
    ratio = float(mag[best] / rest.max()) if rest.max() > 0 else np.inf
    return (best + SYM - 15) % SYM, complex(v[best]), ratio


# ---- the pieces ------------------------------------------------------------------------------------------------------------------------------------
def wrap(th):
    return th - 2 * np.pi * np.rint(th / (2 * np.pi))


def rounded_step(pair):
    """the angle of a float complex increment: what the block turns by per sample"""
    return float(np.arctan2(float(pair[1]), float(pair[0])))


def spectra(x, samperr, theta, dtheta):
    """NCO mix, prefix fold with the pulse shape (rotated by 121 samples: phases referenced to the symbol centre, acquire.c:239-247), 256-point DFT -> [32, 256], FFT order"""
    j = np.arange(SYM)[None, :] + SYM * np.arange(NSYM)[:, None]
    v = np.exp(1j * (theta + dtheta * j)) * x[j + samperr] * SHAPE[None, :]
    folded = v[:, :FFT].copy()
    folded[:, :CP] += v[:, FFT:]
    return np.fft.fft(np.roll(folded, (FFT - CP) // 2, axis=1), axis=1)


def half_turn_diff(a, b):
    """phase_diff, sync.c:284-290 -> (difference, wraps taken)"""
    d, n = a - b, 0
    while d > np.pi / 2:
        d -= np.pi; n += 1
    while d < -np.pi / 2:
        d += np.pi; n += 1
    return d, n


def _slice(f, bounds, codes):
    k = np.searchsorted(bounds, f, side="right")                 # f < b goes below b: the boundary itself belongs to the upper interval
    return codes[k], np.abs(f[..., None] - bounds).min(axis=-1)


def sym_qam64(c):
    a, da = _slice(c.real, _B8, _SLICE8); b, db = _slice(c.imag, _B8, _SLICE8)
    return a | (b << 3), np.minimum(da, db)


def sym_qam16(c):
    a, da = _slice(c.real, _B4, _SLICE4); b, db = _slice(c.imag, _B4, _SLICE4)
    return a | (b << 2), np.minimum(da, db)


def sym_qpsk(c):
    return ((c.real >= 0).astype(np.uint8) | ((c.imag >= 0).astype(np.uint8) << 1)), np.minimum(np.abs(c.real), np.abs(c.imag))


def find_ref(d):
    """find_ref_am (sync.c:240-252) on the 32-bit mask (bit n = symbol n): the first rotation r whose 23 leading positions match, or -1"""
    for r in range(NSYM):
        rot = ((d >> r) | (d << (32 - r))) & 0xffffffff
        if rot & CARE23 == VAL23:
            return r
    return -1


def find_block(d):
    """find_block_am (sync.c:209-238): -1, or the block count of a valid sequence"""
    if d & CARE23 != VAL23:
        return -1
    for group in PARITY_GROUPS:
        if sum((d >> k) & 1 for k in group) & 1:
            return -1
    return (((d >> 17) & 1) << 2) | (((d >> 18) & 1) << 1) | ((d >> 19) & 1)


def partition_bins(ma3):
    """carrier offsets [4 (pl, pu, s, t), 25] and the training cells' ideal sums"""
    col = np.arange(PW)
    pri, ter = (2, 28) if ma3 else (57, 2)
    off = np.stack([-(pri + col), pri + col, 28 + col, -(ter + col) if ma3 else ter + col])
    ideal = np.array([5 - 5j, 5 - 5j, 5 - 5j if ma3 else 3 - 1j, 5 - 5j if ma3 else -1 + 1j])
    return off, ideal


def pids_gather(pids_sym, disabled):
    """decode.c:476-501: 64 QAM16 codes (2 n = the first PIDS carrier of symbol n, 2 n + 1 = the second) -> 240 trellis inputs"""
    out = np.zeros(240, dtype=np.int8)
    for n in range(120):
        p = n % 4
        k = (n + n // 60 + 11) % 30; row = (11 * (k + k // 15) + 3) % 32
        il = (pids_sym[2 * row] >> p) & 1
        k = (n + n // 60) % 30; row = (11 * (k + k // 15) + 3) % 32
        iu = (pids_sym[2 * row + 1] >> p) & 1
        i, j = n // 12, n % 12
        out[24 * i + PIDS_IL_POS[j]] = 0 if disabled else (1 if il else -1)
        out[24 * i + PIDS_IU_POS[j]] = 1 if iu else -1
    return out


# ---- one block ---------------------------------------------------------------------------------------------------------------------------------------
def block(win, state, hist=None, fill=WIN):
    """win int16 [8910, 2]; state: the words of STATE_DEFAULTS (missing: as a fresh session); hist int16 [31, 2] (needed while not FINE) -> dict(rec, state, ...)"""
    st = dict(STATE_DEFAULTS); st.update(state)
    out = dict(state=st, active=int(fill >= WIN))
    st["active"] = out["active"]
    if not out["active"]:
        return out
    x = q15_to_c(win)
    before = st["sync_state"]
    rec = dict(flags=REC_PROCESSED, state_before=before, freq_offset=0.0, bc_decoded=-1, sis=0, p1_slot=-1)
    # 1. bookkeeping and angle (acquire.c:110-119, 153-168)
    prev = float(f32(st["prev_angle"]))
    if before == FINE:
        samperr = SYM // 2 + st["samperr"]; st["samperr"] = 0
        angle = float(f32(prev - st["angle"])); st["angle"] = 0.0
    else:
        samperr, peak, out["acq_ratio"] = acquire(win, hist)
        st["coarse_samperr"], st["coarse_re"], st["coarse_im"] = samperr, peak.real, peak.imag
        diff = np.angle(peak * np.exp(-1j * prev))
        angle = float(f32(prev + diff * (0.25 if prev != 0.0 else 1.0)))
        if before != COARSE:
            rec["flags"] |= REC_TO_COARSE; st["sync_state"] = COARSE
    st["prev_angle"] = angle
    top_state = st["sync_state"]
    angle = float(f32(angle - 2 * np.pi * st["cfo"]))                               # acquire.c:164
    dth = f32(f32(angle) / f32(FFT))
    theta = wrap(st["theta"] + float(f32(-f32(SYM // 2 - samperr) * f32(angle) / f32(FFT))))   # acquire.c:166
    inc = (f32(np.cos(np.float64(dth))), f32(np.sin(np.float64(dth))))              # cexpf(angle / fft * I), a float complex
    # 2-6. pass 1: the analog carrier's phase per symbol, line fit, and the strongest bin near the centre while not FINE (acquire.c:170-235)
    x1 = spectra(x, samperr, theta, rounded_step(inc))
    car = x1[:, 0]
    y = np.cumsum(np.concatenate([[np.angle(car[0])], np.angle(car[1:] / car[:-1])]))
    xs = SYM * (np.arange(NSYM) - (NSYM - 1) / 2)
    slope = (xs * y).sum() / (xs * xs).sum()
    a = -y.sum() / NSYM + slope * NSYM * SYM / 2
    if top_state != FINE:
        mags = np.abs(x1[:, np.arange(-53, 54) % FFT]).sum(axis=0)
        best = int(np.argmax(mags))
        out["cfo_ratio"] = float(mags[best] / np.delete(mags, best).max())
        st["cfo"] += best - 53                                                     # acquire_cfo_adjust: effective from the next block
    theta = wrap(theta + (a - 0.06))                                               # acquire.c:233-234
    rs, rc = f32(np.sin(-np.float64(f32(slope)))), f32(np.cos(-np.float64(f32(slope))))
    inc2 = (f32(f32(inc[0] * rc) - f32(inc[1] * rs)), f32(f32(inc[0] * rs) + f32(inc[1] * rc)))       # phase_increment *= cexpf(-slope I), float complex
    dtheta = rounded_step(inc2)
    # 7-8. pass 2 and the sideband combine (acquire.c:237-257, sync.c:616-633)
    X = spectra(x, samperr, theta, dtheta)
    out["spectra_raw"] = X.copy()                                                  # what the transform leaves (the oracle's TAP_FFT, before its fftshift)
    ma3 = st["psmi"] == MA3
    i = np.arange(1, 82)
    X[:, -i] = -np.conj(X[:, -i])
    if not ma3:
        X[:, 1:54] += X[:, -np.arange(1, 54)]
    out["spectra"] = X.copy()
    # 9-10. reference bits, find_ref_am / find_block_am
    d = int(sum(1 << n for n in range(NSYM) if X[n, 1].imag > 0))
    out["refmask"] = d
    out["ref_dist"] = float(np.abs(X[:, 1].imag).min())
    if top_state == COARSE and st["cfo_wait"] == 0:
        off = find_ref(d)
        if off > 0:
            st["keep_extra"] = ((NSYM - off) % NSYM) * SYM; st["cfo_wait"] = 8
    else:
        st["cfo_wait"] -= 1
    if top_state == COARSE:
        bc = find_block(d)
        if bc == 0:
            st["psmi"] = sum(((d >> (26 + k)) & 1) << (4 - k) for k in range(5))
            st["rdbi"], st["pli"], st["hppi"], st["aabi"] = (d >> 15) & 1, (d >> 7) & 1, (d >> 11) & 1, (d >> 12) & 1
        history = 0 if bc == -1 else ((st["offset_history"] << 4) | bc) & 0xffffffff
        if history & 0xffff == 0x5670:
            st["bc"] = 0; st["sync_state"] = FINE; st["fine_epoch"] += 1
            rec["flags"] |= REC_TO_FINE
            rec["freq_offset"] = (st["prev_angle"] - 2 * np.pi * st["cfo"]) * FS / (2 * np.pi * FFT)
            rec["sis"] = (st["pli"] & 1) | ((st["hppi"] & 1) << 1) | ((st["aabi"] & 1) << 2) | ((st["rdbi"] & 1) << 3) | 16
            st["am_errors"] = 0; st["am_diversity_wait"] = 4
            history = 0
        st["offset_history"] = history
    if st["sync_state"] == FINE:
        ma3 = st["psmi"] == MA3
        bc = st["bc"]
        # 11. the PIDS carriers (sync.c:661-678)
        offs = (-27, 27) if ma3 else (27, 53)
        pids_sym, pids_dist = np.zeros(2 * NSYM, dtype=np.uint8), np.zeros(2 * NSYM)
        out["pids_train"] = np.array([abs(X[8, o] + X[24, o]) / 2 for o in offs])
        for which, o in enumerate(offs):
            m = (3 - 1j) / (X[8, o] + X[24, o])
            pids_sym[which::2], pids_dist[which::2] = sym_qam16(X[:, o] * m)
        # 12. the equaliser taps from the two training cells of each carrier (sync.c:689-714)
        off, ideal = partition_bins(ma3)
        col = np.arange(PW)
        t1, t2 = (5 + 11 * col) % 32, (21 + 11 * col) % 32
        mult = ideal[:, None] / (X[t1[None, :], off] + X[t2[None, :], off])
        out["mult"] = mult
        out["train"] = np.abs(X[t1[None, :], off] + X[t2[None, :], off]) / 2       # mean training-cell magnitude per carrier [4, 25]
        # 13. the timing estimate (sync.c:738-767)
        marg = np.angle(mult[:2])
        se, wraps, wrap_dist = 0.0, 0, np.inf
        for c in range(1, PW):
            for p in range(2):
                dd, n = half_turn_diff(marg[p, c], marg[p, c - 1]); se += dd; wraps += n
                wrap_dist = min(wrap_dist, abs(abs(marg[p, c] - marg[p, c - 1]) - np.pi / 2), abs(abs(marg[p, c] - marg[p, c - 1]) - 3 * np.pi / 2))
        out["wrap_dist"] = float(wrap_dist)                                       # how far the nearest tap-angle difference is from a wrap threshold, rad
        se = se / (2 * (PW - 1)) * FFT / (2 * np.pi)
        st["samperr"] = int(np.sign(se) * np.floor(np.abs(se) + 0.5))              # roundf: halves away from zero
        out["se"], out["se_dist"], out["wraps"] = se, float(np.abs(np.abs(se - np.floor(se)) - 0.5)), wraps
        # 14. equalise and slice the four partitions (sync.c:716-736)
        sym, dist = np.zeros((4, NSYM, PW), dtype=np.uint8), np.zeros((4, NSYM, PW))
        for part in range(4):
            v = X[:, off[part]] * mult[part][None, :]
            sym[part], dist[part] = sym_qam64(v) if part < 2 or ma3 else sym_qam16(v) if part == 2 else sym_qpsk(v)
        out.update(sym=sym.reshape(4, -1), dist=dist.reshape(4, -1), pids_sym=pids_sym, pids_dist=pids_dist)
        # 15. the PIDS bit gather (decode.c:476-501)
        out["pids_coded"] = pids_gather(pids_sym, st["psmi"] == 1 and bool(st["rdbi"]))
        rec["flags"] |= REC_PIDS; rec["bc_decoded"] = bc
        if bc == 0:
            st["am_errors"] = 0
        st["bc"] = (bc + 1) % 8
    # tail (acquire.c:259-262)
    st["theta"] = float(wrap(theta + dtheta * (NSYM * SYM)))
    keep = SYM + (SYM // 2 - samperr) + st["keep_extra"]
    st["keep_extra"] = 0
    st["rd"] += WIN - keep
    st["nblocks"] += 1
    rec.update(state_after=st["sync_state"], samperr=samperr, cfo=st["cfo"], keep=keep, bc=st["bc"], psmi=st["psmi"], cfo_wait=st["cfo_wait"], next_samperr=st["samperr"],
               prev_angle=st["prev_angle"], phase_re=float(np.cos(st["theta"])), phase_im=float(np.sin(st["theta"])), next_angle=st["angle"])
    out["rec"] = rec
    return out


def receive(q15, nblocks=None):
    """the model as a receiver: block after block over a Q15 stream [n, 2], as acquire_push feeds windows (acquire.c:98-109, 259-262) -> the blocks' results"""
    st, hist, pos, outs = dict(STATE_DEFAULTS), np.zeros((31, 2), dtype=np.int16), 0, []
    while pos + WIN <= len(q15) and (nblocks is None or len(outs) < nblocks):
        win = q15[pos:pos + WIN]
        fine = st["sync_state"] == FINE
        o = block(win, st, hist)
        if not fine:
            hist = win[-31:]
        st = dict(o["state"])
        pos += WIN - o["rec"]["keep"]
        outs.append(o)
    return outs
