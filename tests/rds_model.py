"""RDS / RBDS of an analog FM host, restated in float64 from its definition (DESIGN.md (p), E .. H) -- the reference of tests/rds_checks.py.
The signal path is written from the definition, not from the kernels: the baseband is the discriminator output times the exact 57 kHz phasor,
the matched filter is the closed-form biphase symbol under a Hann window at the exact fractional offset of every grid point, timing and
decisions are feed-forward per window of 152 bits.  dtype=np.float32 runs that path in float32 (the taps summed one after the other, as the
definition writes the sum; the window energies in the order the definition fixes, which is the kernel's lane layout and butterfly): the
reference's own estimate of what float32 costs.

How independent it is.  Blocks, groups and content (Groups) follow the same written rules as k_rds_groups and hold the same state -- the ring
of (class, run), the expected class, the bit count of the block, the run of invalid blocks, the group mask -- so a rule misread once would be
misread on both sides.  What anchors it from outside: check words against long division worked out in the test, the source's own bits coming
back from the signal, and the assertions on decoded content (PI, name, text, clock equal what was sent) in tests/rds_args.py."""
import numpy as np

from tests import fm_model as fm

DEN = 11907                      # 19 kHz = 608 / DEN, 57 kHz = 1824 / DEN cycles per Fs1 sample
SC_NUM = 1824
S = 8                            # grid points per bit
GRID = 304                       # grid point r at 11907 r / 304 samples (38 bits = 11907 samples)
T_BIT = DEN / 38.0               # Fs1 samples per bit
HALF = 627                       # taps at j = -HALF .. HALF around floor(t_r): every |m - t_r| <= 2 T is among them
NT = 2 * HALF + 1
WIN_BITS = 152
WIN_PTS = WIN_BITS * S           # 1216 grid points = 47 628 samples
POLY = 0x5B9
OFFSETS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)      # A, B, C, C', D
CLASS_OFFSETS = ((0x0FC,), (0x198,), (0x168, 0x350), (0x1B4,))
LOSS_BLOCKS = 16
KINDS = (None, "pi", "ps", "rt", "clock", "group")
STATS = (("bits", "blocks_valid", "blocks_corrected", "blocks_invalid", "groups", "groups_dropped", "syncs_gained", "syncs_lost", "seam_drops",
          "seam_inserts") + tuple("g%d%s" % (t, v) for t in range(16) for v in "AB") + ("events",))


def h(u):
    return np.sinc(u + 0.5) + np.sinc(u - 0.5)


def design_taps() -> np.ndarray:
    """float64 [GRID][NT]: tap j - HALF of phase ph weighs v[floor(t_r) + j - HALF], tau = j - HALF - ph / 304 samples from the grid point"""
    ph = np.arange(GRID, dtype=np.float64)[:, None]
    tau = np.arange(-HALF, HALF + 1, dtype=np.float64)[None, :] - ph / GRID
    t = tau + T_BIT / 4                                    # g is centred at T / 4
    g = h(4 * t / T_BIT) - h(4 * (t - T_BIT / 2) / T_BIT)
    win = np.where(np.abs(tau) <= 2 * T_BIT, 0.5 * (1 + np.cos(np.pi * tau / (2 * T_BIT))), 0.0)
    return g * win


def points_total(m_total: int) -> int:
    """grid points whose last tap lies inside m_total samples of d"""
    if m_total < HALF + 1:
        return 0
    return (GRID * (m_total - HALF - 1) + GRID - 1) // DEN + 1


def windows_total(m_total: int) -> int:
    return points_total(m_total) // WIN_PTS


LATENCY_IN = 2 * (DEN * (WIN_PTS - 1) // GRID + HALF + 1) - 1      # input samples behind which window 0 is decided; window w: + 2 * 47628 w


def matched(d: np.ndarray, tab: np.ndarray, dtype=np.float64) -> np.ndarray:
    """d [m_total] -> y complex [points_total]; tab as the library stores it (float32 [GRID][NT])"""
    ct = np.complex128 if dtype == np.float64 else np.complex64
    m = np.arange(d.size, dtype=np.int64)
    ang = 2 * np.pi * ((SC_NUM * m) % DEN) / DEN
    e = (np.cos(ang).astype(dtype) - 1j * np.sin(ang).astype(dtype)).astype(ct)
    v = (d.astype(dtype) * e).astype(ct)
    nr = points_total(d.size)
    r = np.arange(nr, dtype=np.int64)
    i0 = (DEN * r) // GRID
    ph = (DEN * r) % GRID
    vp = np.concatenate([np.zeros(HALF, ct), v])            # samples in front of the stream are zero
    tab = np.asarray(tab, dtype=np.float32).astype(dtype)
    y = np.zeros(nr, ct)
    if dtype == np.float64:
        for a in range(0, nr, 512):
            idx = i0[a:a + 512, None] + np.arange(NT)[None, :]
            y[a:a + 512] = np.sum(vp[idx] * tab[ph[a:a + 512]], axis=1)
        return y
    re, im = np.zeros(nr, np.float32), np.zeros(nr, np.float32)
    for j in range(NT):                                     # one tap after the other
        x = vp[i0 + j]
        t = tab[ph, j]
        re = (re + t * x.real).astype(np.float32)
        im = (im + t * x.imag).astype(np.float32)
    return (re + 1j * im).astype(ct)


def decide(y: np.ndarray, dtype=np.float64):
    """-> {"energy" [windows][8], "s" [windows], "bits": list per window of uint8 arrays, "metric": list per window of the decision metrics,
    "drops", "inserts"} for the complete windows of y"""
    nw = y.size // WIN_PTS
    p = (y.real.astype(dtype) ** 2 + y.imag.astype(dtype) ** 2).astype(dtype)
    energy = np.zeros((nw, S), dtype)
    s = np.zeros(nw, np.int64)
    bits, metric = [], []
    drops = inserts = 0
    last = None                                             # grid index of the last sampling point
    for w in range(nw):
        e = p[w * WIN_PTS:(w + 1) * WIN_PTS].reshape(WIN_BITS, S)
        if dtype == np.float64:
            energy[w] = e.sum(axis=0)
        else:                                               # lanes 8 g + s sum bits g, g + 8, ... in order, then a butterfly over g
            part = np.zeros((8, S), np.float32)
            for k in range(WIN_BITS // 8):
                part = (part + e[8 * k:8 * k + 8]).astype(np.float32)
            for step in (1, 2, 4):
                part = (part + part[np.arange(8) ^ step]).astype(np.float32)
            energy[w] = part[0]
        s[w] = int(np.argmax(energy[w]))                    # ties to the lowest s
        pts = [w * WIN_PTS + S * k + int(s[w]) for k in range(WIN_BITS)]
        if w > 0:
            gap = S + int(s[w]) - int(s[w - 1])
            if gap < 4:
                pts = pts[1:]
                drops += 1
            elif gap > 12:
                pts = [last + S] + pts
                inserts += 1
        prev = ([last] if last is not None else pts[:1]) + pts[:-1]
        if last is None:
            pts, prev = pts[1:], prev[1:]                   # the first point of a session has no predecessor
        a, b = y[np.array(pts)], y[np.array(prev)]
        mt = (a.real.astype(dtype) * b.real.astype(dtype) + a.imag.astype(dtype) * b.imag.astype(dtype)).astype(dtype)
        bits.append((mt < 0).astype(np.uint8))
        metric.append(mt)
        last = (w + 1) * WIN_PTS - S + int(s[w])
    return {"energy": energy, "s": s, "bits": bits, "metric": metric, "drops": drops, "inserts": inserts}


def syndrome(word26: int) -> int:
    reg = word26
    for k in range(25, 9, -1):
        if reg >> k & 1:
            reg ^= POLY << (k - 10)
    return reg & 0x3FF


def error_table(burst: int) -> dict:
    """syndrome -> error mask, for single bits (burst >= 1) and two neighbouring bits (burst >= 2)"""
    out = {}
    masks = ([1 << p for p in range(26)] if burst >= 1 else []) + ([3 << p for p in range(25)] if burst >= 2 else [])
    for mk in masks:
        sy = syndrome(mk)
        assert sy not in out and sy != 0
        out[sy] = mk
    return out


class Groups:
    """H: blocks, groups and content of one station's bit stream"""

    def __init__(self, burst: int = 2, raw: bool = False):
        self.burst, self.raw = burst, raw
        self.table = error_table(burst)
        self.events = []
        self.reset()

    def reset(self):
        self.stats = dict.fromkeys(STATS, 0)
        self.nbits = 0
        self.reg = 0
        self.synced = False
        self.ring = [(-1, 0)] * 26                          # (class, run length) of the word that ended at this position mod 26
        self.exp = self.fill = self.bad_run = 0
        self.in_group = False
        self.gw, self.gmask, self.ngroups, self.gindex = [0, 0, 0, 0], 0, 0, 0
        self.pi = -1
        self.pty = self.tp = self.ta = self.ms = self.di = 0
        self.ps_buf, self.ps_mask, self.ps_last = bytearray(8), 0, None
        self.rt_buf, self.rt_mask, self.rt_ab, self.rt_ver, self.rt_last = bytearray(64), 0, -1, -1, None
        self.clock = None

    def snapshot(self) -> dict:
        return {"pi": self.pi, "pty": self.pty, "tp": self.tp, "ta": self.ta, "ms": self.ms, "di": self.di, "synced": int(self.synced),
                "ps": None if self.ps_last is None else bytes(self.ps_last), "rt": None if self.rt_last is None else bytes(self.rt_last),
                "rt_ab": self.rt_ab, "clock": self.clock}

    def _event(self, kind: str, v, data: bytes = b""):
        v = list(v) + [0] * (8 - len(v))
        self.events.append({"kind": kind, "group": self.gindex, "bit": self.nbits - 1, "v": v, "data": bytes(data)})
        self.stats["events"] += 1

    def push(self, bits):
        for b in bits:
            self._bit(int(b) & 1)
        return self

    def _bit(self, b: int):
        idx = self.nbits
        self.nbits += 1
        self.stats["bits"] += 1
        self.reg = (self.reg << 1 | b) & 0x3FFFFFF
        syn = syndrome(self.reg)
        if not self.synced:
            cls = -1
            if idx >= 25:
                for c, offs in enumerate(CLASS_OFFSETS):
                    if syn in offs:
                        cls = c
            run = 0
            if cls >= 0:
                pc, pr = self.ring[idx % 26]
                run = pr + 1 if pr > 0 and pc == (cls + 3) % 4 else 1
            self.ring[idx % 26] = (cls, run)
            if run >= 3:
                self.synced = True
                self.stats["syncs_gained"] += 1
                self.exp, self.fill, self.bad_run, self.in_group = (cls + 1) % 4, 0, 0, False
                self.ring = [(-1, 0)] * 26
            return
        self.fill += 1
        if self.fill == 26:
            self.fill = 0
            self._block(self.exp, self.reg, syn)
            self.exp = (self.exp + 1) % 4

    def _block(self, cls: int, reg: int, syn: int):
        ok, word = False, reg >> 10
        for x in CLASS_OFFSETS[cls]:
            if syn == x:
                ok = True
        if ok:
            self.stats["blocks_valid"] += 1
            self.bad_run = 0
        else:
            for x in CLASS_OFFSETS[cls]:
                mk = self.table.get(syn ^ x)
                if mk is not None:
                    ok, word = True, (reg ^ mk) >> 10
                    break
            self.stats["blocks_corrected" if ok else "blocks_invalid"] += 1
            if not ok:
                self.bad_run += 1                           # a corrected block neither counts nor ends the run
        if cls == 0:
            self.in_group, self.gmask, self.gindex = True, 0, self.ngroups
            self.ngroups += 1
        if self.in_group and ok:
            self.gw[cls] = word
            self.gmask |= 1 << cls
        if cls == 3 and self.in_group:
            self.in_group = False
            if self.gmask == 15:
                self._group(*self.gw)
            else:
                self.stats["groups_dropped"] += 1
        if self.bad_run >= LOSS_BLOCKS:
            self.synced, self.in_group = False, False
            self.stats["syncs_lost"] += 1
            self.ring = [(-1, 0)] * 26

    def _set_pi(self, v: int):
        if v != self.pi:
            self.pi = v
            self.ps_mask, self.ps_last = 0, None
            self.rt_mask, self.rt_ab, self.rt_ver, self.rt_last = 0, -1, -1, None
            self._event("pi", [v])

    def _group(self, a: int, b: int, c: int, d: int):
        gt, ver = b >> 12, b >> 11 & 1
        self.stats["groups"] += 1
        self.stats["g%d%s" % (gt, "AB"[ver])] += 1
        if self.raw:
            self._event("group", [a, b, c, d])
        self._set_pi(a)
        if ver:
            self._set_pi(c)
        self.pty, self.tp = b >> 5 & 31, b >> 10 & 1
        if gt == 0:
            seg = b & 3
            self.ta, self.ms = b >> 4 & 1, b >> 3 & 1
            self.di = self.di & ~(1 << (3 - seg)) | (b >> 2 & 1) << (3 - seg)
            self.ps_buf[2 * seg], self.ps_buf[2 * seg + 1] = d >> 8, d & 255
            self.ps_mask |= 1 << seg
            if self.ps_mask == 15 and self.ps_last != self.ps_buf:
                self.ps_last = bytearray(self.ps_buf)
                self._event("ps", [self.pi], self.ps_last)
        elif gt == 2:
            flag, seg = b >> 4 & 1, b & 15
            if flag != self.rt_ab or ver != self.rt_ver:
                self.rt_buf, self.rt_mask, self.rt_ab, self.rt_ver = bytearray(64), 0, flag, ver
            per = 2 if ver else 4
            chars = (d >> 8, d & 255) if ver else (c >> 8, c & 255, d >> 8, d & 255)
            self.rt_buf[per * seg:per * seg + per] = bytes(chars)
            self.rt_mask |= 1 << seg
            length = 0
            for sg in range(16):
                if not self.rt_mask >> sg & 1:
                    break
                if 0x0D in self.rt_buf[per * sg:per * sg + per] or sg == 15:
                    length = sg + 1
                    break
            if length:
                text = bytearray(self.rt_buf[:per * length])
                if self.rt_last != text:
                    self.rt_last = text
                    self._event("rt", [self.pi, flag], text)
        elif gt == 4 and ver == 0:
            off = d & 31
            key = ((b & 3) << 15 | c >> 1, (c & 1) << 4 | d >> 12, d >> 6 & 63, -off if d >> 5 & 1 else off)
            if key != self.clock:
                self.clock = key
                self._event("clock", list(key))


def receive(x: np.ndarray, ha: np.ndarray, tab: np.ndarray, dtype=np.float64, burst: int = 2, raw: bool = False) -> dict:
    """one channel, cs16 [n, 2] -> everything the checks compare: d, y, energy, s, bits (per window and joined), the decoder"""
    d, _ = fm.front(x, np.asarray(ha, dtype=np.float32).astype(dtype), dtype)
    y = matched(d, tab, dtype)
    out = decide(y, dtype)
    out["d"], out["y"] = d, y
    out["stream"] = np.concatenate(out["bits"]) if out["bits"] else np.zeros(0, np.uint8)
    g = Groups(burst, raw).push(out["stream"])
    g.stats["seam_drops"], g.stats["seam_inserts"] = out["drops"], out["inserts"]
    out["groups"] = g
    return out
