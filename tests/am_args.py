"""The input sets of the AM block-step stage tests (tests/am_checks.py): one hook call = one block = one Case.  Written once, fixed seeds, noise-free unless a set
is about noise.  Windows are synthesised from nrsc5_amd.synth_am (block_spectrum / block_spectrum_ma3, reference_bits, ofdm_modulate): 35 symbols, cut so that symbol
0 of the block starts `start` samples into the 8910-sample window, scaled to ~20 LSB rms (one set: full scale) and rounded to Q15.

  refseq    COARSE, integer logic: every rotation of the reference sequence, every block count, single violations of find_ref_am / find_block_am, offset_history
  cells     FINE: every constellation point on every carrier of every partition, flat and smooth channels with a timing offset, samperr at both ends, carrier phase
  edge      the cells signal plus noise (a known share of cells near a slicer boundary) and a channel whose tap angles step across pi / 2 (half_turn_diff wraps)
  carrier   NONE / COARSE: the integer carrier offset at -53 .. +53 bins and fractions of a bin, the symbol start at 0 / 15 / 269, prev_angle zero and not
  inactive  a window that is a sample short

THE TOLERANCES (nothing here is measured on the kernel under test):
  SPEC_ERR_MEASURED  the oracle's float32 spectra (TAP_FFT: the reference's own arithmetic, bit for bit -- a float oscillator recurrence and a float FFT) against the
                     float64 model over every block of the two pin captures, bins -81 .. +81, largest error relative to the block's largest bin magnitude (the analog
                     carrier): am_cs16_cfo3 1.92e-5, am_ma3_cs16 7.2e-6.  tests/test_am_block_stage_cpu.py asserts the oracle stays within it.
  SPEC_FACTOR        the device gets 4 x that: another, equally valid float32 factorisation (16 x 16 transform, closed-form oscillator heads every eight symbols).
  margins()          SPEC_BOUND carried through the equaliser.  With eps = SPEC_BOUND * (largest bin) the absolute error of a bin, a cell v = X * ideal / T
                     (T = the sum of the carrier's two training cells, |T| = 2 t) is off by at most eps |ideal| / |T| + |v| 2 eps / |T| = eps (|ideal| + 2 |v|max) / (2 t)
                     grid units; a tap's angle by 2 eps / |T| = eps / t rad; the sum of the 24 tap-angle differences of a sideband telescopes to last - first, so
                     `se` is off by at most 4 (eps / t) / 48 * 256 / (2 pi) samples, as long as no difference crosses a wrap threshold: a difference is off by 2 eps / t.
Measured with these constants (model alone, tests/test_am_block_stage_cpu.py prints them): cell margins 1e-3 .. 1e-2 grid units; no cell of any set but `edge` is
within its margin, 0.2 % .. 1 % of the cells of an `edge` call are."""
import dataclasses
import functools

import numpy as np

from nrsc5_amd import synth_am as sa
from tests import am_model as M

SPEC_ERR_MEASURED = 2.0e-5                 # measured 1.92e-5 (see above), rounded up
SPEC_FACTOR = 4.0
SPEC_BOUND = SPEC_FACTOR * SPEC_ERR_MEASURED
RMS_LSB = 20.0
NONE, COARSE, FINE = M.NONE, M.COARSE, M.FINE
# (|ideal| + 2 |v|max) / 2 per constellation: QAM64 (training 2.5 - 2.5j, corner 3.5 + 3.5j), QAM16 (1.5 - 0.5j, 1.5 + 1.5j), QPSK (-0.5 + 0.5j, 0.5 + 0.5j)
K_QAM64 = (abs(5 - 5j) + 2 * abs(3.5 + 3.5j)) / 2
K_QAM16 = (abs(3 - 1j) + 2 * abs(1.5 + 1.5j)) / 2
K_QPSK = (abs(-1 + 1j) + 2 * abs(0.5 + 0.5j)) / 2
TAUS = (-2.0, -1.0, -0.4, 0.0, 0.4, 1.0, 2.0)
EDGE_SHARE = (0.002, 0.01)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    win: np.ndarray            # int16 [8910, 2]
    hist: np.ndarray           # int16 [31, 2]
    state: dict                # the words the hook writes (missing: a fresh session's)
    fill: int = M.WIN
    sent: dict = None          # what was transmitted: the four code matrices [32, 25], PIDS codes [2, 32]


# ---- the signal ----------------------------------------------------------------------------------------------------------------------------------------
def train_rows(col):
    return (5 + 11 * col) % 32, (21 + 11 * col) % 32


def data_rows():
    """[25, 30]: the rows of every column that carry data"""
    return np.array([[n for n in range(32) if n not in train_rows(c)] for c in range(25)])


def matrices(psmi, kind, k=0, seed=0):
    """code matrices pl, pu, s, t [32, 25] and PIDS codes [2, 32] with the training cells in place.  kind "cover": data cell i (0 .. 29) of column c holds code
    (i + 30 k + 7 c + partition) mod the constellation size, so that calls k = 0 .. 7 put every point on every carrier; "random": uniform"""
    ma3 = psmi == M.MA3
    sizes = (64, 64, 64 if ma3 else 16, 64 if ma3 else 4)
    trains = (sa.TRAIN_QAM64, sa.TRAIN_QAM64, sa.TRAIN_QAM64 if ma3 else sa.TRAIN_QAM16, sa.TRAIN_QAM64 if ma3 else sa.TRAIN_QPSK)
    rng = np.random.default_rng(1000 + seed)
    rows = data_rows()
    mats = []
    for p, (size, train) in enumerate(zip(sizes, trains)):
        m = np.full((32, 25), train, dtype=np.uint8)
        for c in range(25):
            m[rows[c], c] = rng.integers(0, size, 30) if kind == "random" else (np.arange(30) + 30 * k + 7 * c + p) % size
        mats.append(m)
    pids = np.full((2, 32), sa.TRAIN_QAM16, dtype=np.uint8)
    prow = [n for n in range(32) if n not in (8, 24)]
    for w in range(2):
        pids[w, prow] = rng.integers(0, 16, 30) if kind == "random" else (np.arange(30) + 30 * k + 5 * w) % 16
    return mats, pids


def channel(tau=0.0, smooth=False, step=None):
    """per-bin complex gain [256] (index 128 + k = carrier k): a timing offset of tau samples (linear phase), a smooth gain of 0.5 .. 2, a phase step (k0, radians)
    from carrier k0 outwards on both sidebands"""
    k = np.arange(-128, 128)
    h = np.exp(2j * np.pi * k * tau / 256)
    if smooth:
        h = h * 2.0 ** np.sin(2 * np.pi * k / 200 + 0.7)
    if step is not None:
        h = h * np.exp(1j * step[1] * (np.abs(k) >= step[0]))
    return h


def window(psmi=1, bc=0, rdbi=0, mats=None, ref=None, h=None, start=40, cfo_bins=0.0, phase=0.0, rate=0.0, noise=0.0, seed=0, fullscale=False):
    """-> (int16 [8910, 2], sent).  ref: the 32 reference bits instead of reference_bits(bc, psmi, rdbi); cfo_bins / phase / rate: the signal is turned by
    exp(j (phase + (2 pi cfo_bins / 256 + rate) n)); noise: complex sigma per sample in grid units"""
    m, pids = mats if mats is not None else matrices(psmi, "cover")
    spec = (sa.block_spectrum_ma3 if psmi == M.MA3 else sa.block_spectrum)(m[0], m[1], m[2], m[3], pids[0], pids[1], bc, rdbi)
    if ref is not None:
        r = 1j * sa.LEVEL_REF * (np.asarray(ref, dtype=np.float64) * 2 - 1)
        spec[:, 129] = r; spec[:, 127] = -np.conj(r)
    if h is not None:
        spec = spec * h[None, :]
    sym = sa.ofdm_modulate(spec).reshape(32, M.SYM)
    sig = np.concatenate([sym[-1], sym.reshape(-1), sym[0], sym[1]])            # symbol 0 of the block starts at sample 270
    sig = sig[M.SYM - start:M.SYM - start + M.WIN].copy()
    n = np.arange(M.WIN)
    sig *= np.exp(1j * (phase + (2 * np.pi * cfo_bins / 256 + rate) * n))
    if noise:
        rng = np.random.default_rng(77 + seed)
        sig += noise * (rng.standard_normal(M.WIN) + 1j * rng.standard_normal(M.WIN)) / np.sqrt(2)
    scale = 32000.0 / max(np.abs(sig.real).max(), np.abs(sig.imag).max()) if fullscale else RMS_LSB / np.sqrt(np.mean(np.abs(sig) ** 2))
    q = np.rint(scale * np.stack([sig.real, sig.imag], axis=1))
    return np.clip(q, -32768, 32767).astype(np.int16), dict(mats=m, pids=pids, psmi=psmi, bc=bc, rdbi=rdbi)


_HIST = np.zeros((31, 2), dtype=np.int16)


def _case(name, state, fill=M.WIN, **kw):
    win, sent = window(**kw)
    return Case(name, win, _HIST if state.get("sync_state", NONE) == FINE else np.ascontiguousarray(win[:31][::-1]), state, fill, sent)


def fine_state(psmi, bc, rdbi, start=40, **more):
    """a FINE stream in front of block bc whose symbols start `start` samples into the window: samperr = start - 135"""
    st = dict(sync_state=FINE, psmi=psmi, bc=bc, rdbi=rdbi, pli=0, hppi=0, aabi=0, samperr=start - M.SYM // 2, am_diversity_wait=2, am_errors=5, cfo_wait=-3)
    st.update(more)
    return st


# ---- the sets ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refseq():
    out = []
    coarse = dict(sync_state=COARSE)
    seq = sa.reference_bits(3)
    for cw in (0, 3):                                                          # every rotation: keep_extra and cfo_wait -> 8, or the decrement
        for r in range(32):
            out.append(_case("rot%d-wait%d" % (r, cw), dict(coarse, cfo_wait=cw, offset_history=0x56), ref=np.roll(seq, r), bc=3, start=40 + r))
    for bc in range(8):                                                        # every block count, both service modes, rdbi
        for psmi in (1, 2):
            for rdbi in (0, 1):
                out.append(_case("bc%d-psmi%d-rdbi%d" % (bc, psmi, rdbi), dict(coarse, cfo_wait=5, offset_history=0x12, psmi=7, rdbi=-1), psmi=psmi, bc=bc, rdbi=rdbi, start=100))
    valid = sa.reference_bits(0)
    for pos in (0, 1, 2, 3, 4, 5, 6, 9, 14, 21, 22):                           # the eleven fixed positions, one flipped
        d = valid.copy(); d[pos] ^= 1
        out.append(_case("care%d" % pos, dict(coarse, cfo_wait=2, offset_history=0x567), ref=d, start=7))
    for pos in (8, 12, 18, 27):                                                # one bit of each parity group
        d = valid.copy(); d[pos] ^= 1
        out.append(_case("parity%d" % pos, dict(coarse, cfo_wait=2, offset_history=0x567), ref=d, start=7))
    system = valid.copy(); system[[7, 8, 11, 12]] ^= 1                          # pli, hppi, aabi set (parities kept): latched at bc 0
    out.append(_case("system-bits", dict(coarse, cfo_wait=1, offset_history=0), ref=system, start=7))
    for name, hist, bc in (("hist567-bc0", 0x567, 0), ("hist0567-bc3", 0x0567, 3), ("hist5670-bc0", 0x5670, 0), ("histf567-bc0", 0xf567, 0), ("hist567-bc0-ma3", 0x567, 0)):
        psmi = 2 if name.endswith("ma3") else 1
        out.append(_case(name, dict(coarse, psmi=psmi, cfo_wait=1, offset_history=hist, bc=5, am_errors=9, am_diversity_wait=1, prev_angle=0.01, cfo=0), psmi=psmi, bc=bc, rdbi=int(psmi == 1 and bc == 0),
                         mats=matrices(psmi, "cover", 1), start=60, rate=-0.01 / 256))
    out.append(_case("fine-wait0", fine_state(1, 2, 0, cfo_wait=0), bc=2))          # the decrement is unconditional: -> -1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cells():
    out = []
    chans = [None] + [dict(tau=t, smooth=True) for t in TAUS]
    for psmi in (1, 2):
        for bc in range(8):
            rdbi = bc & 1 if psmi == 1 else 0
            ch = chans[(bc + 4 * (psmi - 1)) % 8]
            # (blocks 0, 6 and 7 behind the diversity delay: the pipeline form announces their frames)
            out.append(_case("psmi%d-bc%d-%s" % (psmi, bc, "flat" if ch is None else "tau%+.1f" % ch["tau"]), fine_state(psmi, bc, rdbi, am_diversity_wait=0 if bc in (0, 6, 7) else 2),
                             psmi=psmi, bc=bc, rdbi=rdbi,
                             mats=matrices(psmi, "cover", bc), h=None if ch is None else channel(**ch)))
        out.append(_case("psmi%d-random" % psmi, fine_state(psmi, 4, 0), psmi=psmi, bc=4, mats=matrices(psmi, "random", seed=psmi), h=channel(0.4, True)))
    for start in (0, 270):                                                     # the samperr state word at both ends of its range
        out.append(_case("start%d" % start, fine_state(1, 1, 0, start=start), bc=1, mats=matrices(1, "cover", 3), start=start))
    out.append(_case("fullscale", fine_state(1, 6, 0), bc=6, mats=matrices(1, "random", seed=9), fullscale=True))
    # a carrier that turns: prev_angle (rad per 256 samples) holds the offset, the line fit the rest; st.angle: what an FM session left (acquire.c:115-118)
    out.append(_case("phase", fine_state(1, 5, 1, prev_angle=0.05, theta=2.5), bc=5, rdbi=1, mats=matrices(1, "cover", 5), phase=1.0, rate=-0.05 / 256 + 2e-6))
    out.append(_case("phase-ma3-angle", fine_state(2, 7, 0, prev_angle=-0.2, angle=0.03, theta=-1.0, cfo=0), psmi=2, bc=7, mats=matrices(2, "cover", 2), phase=-2.0,
                     rate=0.23 / 256, h=channel(-1.0, True)))
    return tuple(out)


EDGE_NOISE = 4.0                           # complex sigma per sample in grid units = 0.25 grid units per cell: 0.3 % .. 0.9 % of an edge call's cells lie within their margin


@functools.lru_cache(maxsize=None)
def edge():
    out = []
    for k, (psmi, bc) in enumerate(((1, 0), (1, 3), (2, 6))):
        out.append(_case("noise-psmi%d-bc%d" % (psmi, bc), fine_state(psmi, bc, 0), psmi=psmi, bc=bc, mats=matrices(psmi, "random", seed=20 + k), noise=EDGE_NOISE, seed=k,
                         h=channel(TAUS[2 * k + 1], True)))
    # tap angles that step by 0.6 pi between two neighbouring primary carriers (MA1: 68 | 69; MA3: 13 | 14): half_turn_diff wraps
    out.append(_case("wrap-ma1", fine_state(1, 2, 0), bc=2, mats=matrices(1, "random", seed=30), h=channel(0.4, True, step=(69, 0.6 * np.pi)), noise=EDGE_NOISE, seed=5))
    out.append(_case("wrap-ma3", fine_state(2, 2, 0), psmi=2, bc=2, mats=matrices(2, "random", seed=31), h=channel(-1.0, True, step=(14, -0.6 * np.pi)), noise=EDGE_NOISE, seed=6))
    return tuple(out)


CARRIER_CFOS = (-53.0, -1.0, 0.0, 1.0, 53.0, 0.3, -0.3)


@functools.lru_cache(maxsize=None)
def carrier():
    out = []
    for k, c in enumerate(CARRIER_CFOS):
        state = dict(sync_state=(NONE, COARSE)[k & 1], cfo_wait=k % 3, cfo=(0, 2, -1)[k % 3])
        out.append(_case("cfo%+.1f" % c, state, bc=k, cfo_bins=c + state["cfo"], start=33, mats=matrices(1, "cover", k)))
    for k, start in enumerate((0, 15, 269)):                                   # the symbol start the correlation finds: coarse_samperr
        out.append(_case("start%d" % start, dict(sync_state=(NONE, COARSE, NONE)[k], prev_angle=(0.0, 0.3, -1.2)[k]), bc=k, start=start, cfo_bins=(0.0, 0.1, -0.2)[k],
                         mats=matrices(1, "cover", k)))
    out.append(_case("ma3-cfo+2", dict(sync_state=COARSE, prev_angle=0.5, theta=1.0), psmi=2, bc=1, cfo_bins=2.07, start=200, mats=matrices(2, "cover", 1)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inactive():
    c = cells()[0]
    return tuple(Case("short-%d-state%d" % (fill, state), c.win, c.hist, dict(c.state, sync_state=state), fill) for fill, state in ((M.WIN - 1, FINE), (0, COARSE), (M.WIN - 1, NONE)))


SETS = dict(refseq=refseq, cells=cells, edge=edge, carrier=carrier, inactive=inactive)


def names(which):
    return [c.name for c in SETS[which]()]


def case(which, name):
    return next(c for c in SETS[which]() if c.name == name)


# ---- the model's answer and the margins, once per case ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(which, name):
    c = case(which, name)
    return M.block(c.win, c.state, c.hist, c.fill)


def margins(exp):
    """-> dict(eps: absolute bound of a bin; for a block that ends FINE: cell [4, 1] and pids [2] in grid units, se in samples, wrap in rad)"""
    eps = SPEC_BOUND * float(np.abs(exp["spectra"]).max())
    out = dict(eps=eps)
    if "sym" in exp:
        ma3 = exp["rec"]["psmi"] == M.MA3
        k = np.array([K_QAM64, K_QAM64, K_QAM64 if ma3 else K_QAM16, K_QAM64 if ma3 else K_QPSK])
        t = exp["train"].min(axis=1)
        out.update(cell=(k * eps / t)[:, None], pids=K_QAM16 * eps / exp["pids_train"], se=4 * (eps / t[:2].min()) / 48 * 256 / (2 * np.pi), wrap=2 * eps / t[:2].min())
    return out


def excluded(exp, mg):
    """the cells within their margin of a slicer boundary [4, 800], and the PIDS cells [64]"""
    return exp["dist"] <= mg["cell"], exp["pids_dist"] <= np.tile(mg["pids"], 32)
