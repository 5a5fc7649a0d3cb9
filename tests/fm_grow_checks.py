"""The checks of the analog FM object's buffers that grow (nrsc5_amd/csrc/fm_host.h: the ping-pong arrays d, p, r, the carrier and impairment
records, RDS's y and SAME's c, and the two event arenas), written once and run twice: by tests/test_fm_grow_cpu.py on the CPU-emulated twin and
by tests/test_gpu_fm_grow.py on gfx950.

Every other FM test session is short enough to fit the capacities an object starts with.  Here one push is long enough that each array has to
grow in the middle of fm_launch, and the reference is the same input pushed in pieces of 100 000 samples on a fresh object, which grows
nothing: growing must not change a byte of what the object delivers, nor add a kernel launch.

The capacities an object starts with are restated below from the host sources; each check asserts that its push is beyond every one of them (and
a piece of the chunked run beyond none), so a session that no longer reaches a path fails instead of passing for nothing."""
import functools

import numpy as np

from nrsc5_amd import synth_fm as sf
from tests import fm_checks as fc, fm_model as fm, impair_checks as ic, rds_args as ra, rds_checks as rc, rds_model as rm, same_args as sa
from tests import same_checks as sc, same_model as sm

# what create / enable allocate beyond the part kept from push to push (fm_audio.hip, fm_carrier.hip, fm_impair.hip, rds.hip, same.hip)
ROOM_D = ROOM_R = 65536                       # Fs1 samples
ROOM_BLOCKS = 256                             # pilot sums, carrier triples, impairment records
ROOM_POINTS = 8192                            # RDS grid points, SAME segments
KEEP_MAX_BLOCKS = 2 * fm.W + 3
RECORDS_KEPT = 2 * fm.W + 1
# the bound of the events nbits more bits can yield, in bytes of a channel's arena (events_bound in rds.hip and same.hip; the constants in rds.h, same.h)
RDS_WIN_MAX_BITS, SAME_WIN_MAX_BITS = rm.WIN_BITS + 1, sm.WIN_BITS + 1


def rds_events_bound(nbits: int) -> int:
    return (nbits // 104 + 2) * 6 * (64 + 64)


def same_events_bound(nbits: int) -> int:
    return (nbits // 48 + 2) * 2 * (64 + 272)


RDS_ARENA_CAP, SAME_ARENA_CAP = rds_events_bound(4 * RDS_WIN_MAX_BITS * 8), same_events_bound(8 * SAME_WIN_MAX_BITS * 8)

N_ARRAYS = 1720000                            # one push of this many input samples grows all seven arrays
N_ARENAS = 6000000                            # ... and of this many both event arenas
CHUNK = 100000
BASE = sa.N                                   # the station is synthesised this long (it holds a whole header burst) and repeated
EVERYTHING = dict(rds=True, same=True, carrier=True, steer=True, impair=True)


@functools.lru_cache(maxsize=None)
def station_base() -> np.ndarray:
    """int16 [BASE, 2]: programme, RDS groups and one SAME header burst"""
    x = sf.fm_host(BASE, amp=ra.AMP, **ra.AUDIO, rds=dict(groups=ra.schedule(ra.PI_A, "KEXP-FM "), dev_hz=2000.0), same=sa._same(2.0, sa.HEADER))
    x.setflags(write=False)
    return x


def station(n: int) -> np.ndarray:
    """the base repeated to n samples: the carrier's phase steps where it repeats, which both runs see alike"""
    return np.tile(station_base(), (-(-n // BASE), 1))[:n]


@functools.lru_cache(maxsize=None)
def two_channels() -> np.ndarray:
    """int16 [2, N_ARRAYS, 2]: the station, and another programme in noise"""
    other = sf.fm_host(N_ARRAYS, amp=ra.AMP, left=[(400.0, 0.25)], right=[(1700.0, 0.15)], preemph_us=75, cnr_db=35.0, seed=3)
    x = np.stack([station(N_ARRAYS), other])
    x.setflags(write=False)
    return x


def thresholds(taps_audio: int) -> dict:
    """array -> (what one push from a fresh object needs of it, given m1 Fs1 samples; the capacity it starts with)"""
    return {
        "d": (lambda m1: m1, KEEP_MAX_BLOCKS * fm.BLOCK + taps_audio + ROOM_D),
        "r": (lambda m1: m1, fm.BLOCK + ROOM_R),
        "p": (lambda m1: m1 // fm.BLOCK, KEEP_MAX_BLOCKS + ROOM_BLOCKS),
        "carrier t": (lambda m1: m1 // fm.BLOCK, RECORDS_KEPT + ROOM_BLOCKS),
        "impair t": (lambda m1: m1 // fm.BLOCK, RECORDS_KEPT + ROOM_BLOCKS),
        "y": (lambda m1: rm.points_total(m1), 2 * rm.WIN_PTS + ROOM_POINTS),
        "c": (lambda m1: sm.segments_total(m1), 2 * sm.WIN_PTS + ROOM_POINTS),
    }


def assert_arrays_grow(n: int, taps_audio: int):
    m1 = (n + 1) // 2
    for name, (need, cap) in thresholds(taps_audio).items():
        assert need(m1) > cap, (name, need(m1), cap)
    # a piece of the chunked run adds less than the room beyond what is kept
    mc = CHUNK // 2 + 1
    assert mc <= ROOM_D and mc // fm.BLOCK + 1 <= ROOM_BLOCKS and rm.points_total(mc) + 1 <= ROOM_POINTS and sm.segments_total(mc) + 1 <= ROOM_POINTS


def assert_arenas_grow(n: int):
    m1 = (n + 1) // 2
    rds_windows, same_windows = rm.points_total(m1) // rm.WIN_PTS, sm.windows_total(sm.segments_total(m1))
    assert rds_events_bound(rds_windows * RDS_WIN_MAX_BITS) > RDS_ARENA_CAP, (rds_windows, RDS_ARENA_CAP)
    assert same_events_bound(same_windows * SAME_WIN_MAX_BITS) > SAME_ARENA_CAP, (same_windows, SAME_ARENA_CAP)


def session(be: fc.Backend, x: np.ndarray, chunks, everything: bool = True) -> dict:
    """a fresh object with everything enabled; push x (int16 [K, n, 2]) in the given chunk sizes (the last one takes the rest) -> all it delivers"""
    k, n = x.shape[0], x.shape[1]
    D = be.demod(k, **EVERYTHING)
    keep_in, p_in = be.upload(x)
    cap = D.outputs_for(n) + 64
    keep_out, p_out = be.zeros((k, cap, 2))
    pos = got = 0
    for c in list(chunks) + [n]:
        c = min(int(c), n - pos)
        if c <= 0:
            break
        got += D.process(p_in + 4 * pos, 2 * n, c, p_out + 4 * got, 2 * cap, cap - got)
        pos += c
    assert pos == n and got == fm.outputs_total(n)
    out = {"launches": D.launches(), "taps_audio": D.taps_audio}
    out["rds_events"], out["same_events"] = rc.split_events(D.rds_read(), k), sc.split_events(D.same_read(), k)
    assert D.rds_read() == [] and D.same_read() == []                           # delivered once
    out["rds_stats"], out["same_stats"] = [D.rds_stats(c) for c in range(k)], [D.same_stats(c) for c in range(k)]
    if everything:
        out["rds_get"], out["same_get"] = [D.rds_get(c) for c in range(k)], [D.same_get(c) for c in range(k)]
        out["pcm"] = be.download(keep_out)[:, :got].tobytes()
        out["clips"] = D.clip_counts().tobytes()
        level, stereo = D.pilot()
        out["pilot"] = (level.tobytes(), stereo.tobytes())
        out["carrier"], out["impair"], out["steer"] = D.carrier(), D.impair(), D.steer()
    D.close()
    return out


def floats_as_bytes(v):
    """the report structures hold floats: compared by their bytes, so that a NaN equals itself and -0.0 differs from 0.0"""
    if isinstance(v, dict):
        return {k: floats_as_bytes(w) for k, w in v.items()}
    if isinstance(v, (list, tuple)):
        return [floats_as_bytes(w) for w in v]
    return np.float64(v).tobytes() if isinstance(v, float) else v


def compare(one: dict, chunked: dict, keys):
    for key in keys:
        a, b = floats_as_bytes(one[key]), floats_as_bytes(chunked[key])
        assert a == b, (key, one[key] if not isinstance(one[key], bytes) else "bytes differ", chunked[key] if not isinstance(chunked[key], bytes) else "")


def launches_one_push(n: int) -> int:
    """the existing helpers' count of a session in one push with everything enabled: growing a buffer is host work and copies, no kernel"""
    return ic.launches_expected([], n, True, True) + rc.expected_launches(n, [], True)[1] + sc.expected_launches(n, [], True)[1]


def check_arrays_grow(be: fc.Backend):
    """two channels, one push that grows d, p, r, both t, y and c once each: everything the object delivers equals the chunked run's"""
    x = two_channels()
    chunked = session(be, x, [CHUNK] * (N_ARRAYS // CHUNK))
    one = session(be, x, [])
    assert_arrays_grow(N_ARRAYS, one["taps_audio"])
    assert one["rds_events"][0] and one["same_events"][0], "the station carries RDS groups and a SAME burst"
    assert one["rds_events"][0] != one["rds_events"][1] and one["pcm"] != bytes(len(one["pcm"]))
    compare(one, chunked, ["pcm", "clips", "pilot", "carrier", "impair", "steer", "rds_events", "same_events", "rds_get", "same_get", "rds_stats", "same_stats"])
    assert one["launches"] == launches_one_push(N_ARRAYS), (one["launches"], launches_one_push(N_ARRAYS))
    assert one["carrier"][0]["blocks"] == (N_ARRAYS + 1) // 2 // fm.BLOCK


def check_arenas_grow(be: fc.Backend):
    """one channel, one push whose bound of unread events is beyond both arenas: the events and the counters equal the chunked run's"""
    assert_arenas_grow(N_ARENAS)
    x = station(N_ARENAS)[None]
    chunked = session(be, x, [CHUNK] * (N_ARENAS // CHUNK), everything=False)
    one = session(be, x, [], everything=False)
    assert one["rds_events"][0] and one["same_events"][0]
    compare(one, chunked, ["rds_events", "same_events", "rds_stats", "same_stats"])
    assert one["launches"] == launches_one_push(N_ARENAS), (one["launches"], launches_one_push(N_ARENAS))
