"""`-m "not gpu"`: RDS on the analog FM object (nrsc5hip_fm_rds_*, nrsc5_amd/csrc/k_rds.hip) on the CPU-emulated twin against the float64
restatement of its definition (tests/rds_model.py); the checks are tests/rds_checks.py, which tests/test_gpu_rds_stage.py runs on gfx950.  The
model itself is pinned first: the source's groups come back bit for bit from a clean signal, and the check words of hand-written blocks equal
what long division by the generator polynomial gives, worked out here."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth_fm as sf
from tests import fm_args as fa, rds_args as ra, rds_checks as rc, rds_model as rm


@pytest.fixture(scope="module")
def be(emu_lib):
    return rc.Backend(emu_lib, gpu=False)


# ---------------------------------------------------------------------------------------------------------- the model and the source
def _divide(word: int) -> int:
    """remainder of word(x) x^10 by x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1, one subtraction of the shifted polynomial per set bit"""
    poly = [10, 8, 7, 5, 4, 3, 0]
    bits = {k + 10 for k in range(16) if word >> k & 1}
    while bits and max(bits) >= 10:
        top = max(bits)
        bits ^= {top - 10 + e for e in poly}
    return sum(1 << k for k in bits)


@pytest.mark.parametrize("word", [0x0000, 0x0001, 0x8000, 0x3AAB, 0x54A9, 0xFFFF, 0x0408, 0xE0CD])
def test_check_words_equal_long_division(word):
    check = _divide(word)
    assert sf.rds_checkword(word) == check
    for off in rm.OFFSETS:
        assert rm.syndrome(word << 10 | (check ^ off)) == off               # valid with offset X: the remainder is X
    assert rm.syndrome(word << 10 | check) == 0
    if word == 0x0001:
        assert check == 0x1B9                                               # x^10 mod g = x^8 + x^7 + x^5 + x^4 + x^3 + 1


def test_error_table_has_distinct_syndromes():
    assert len(rm.error_table(1)) == 26 and len(rm.error_table(2)) == 51 and not rm.error_table(0)


def _parent_fm_host(n, left=(), right=(), pilot=0.1, pilot_ppm=0.0, pilot_phase=0.3, preemph_us=None, amp=8000.0, cnr_db=None, seed=0):
    """fm_host as it was before the keyword `rds` existed, restated: the closed-form phase integral of the MPX's sinusoids, term by term in the same order"""
    terms = []
    for sign_d, tones in ((1.0, left), (-1.0, right)):
        for t in tones:
            f, a, ph = float(t[0]), float(t[1]), (float(t[2]) if len(t) > 2 else 0.0)
            if preemph_us:
                a *= float(np.sqrt(1.0 + (2 * np.pi * f * preemph_us * 1e-6) ** 2))
            terms.append((0.9 * a / 2, f, ph + np.pi / 2))
            if pilot is not None:
                fs2, th2 = 2 * sf.PILOT_HZ * (1 + pilot_ppm * 1e-6), 2 * pilot_phase
                terms.append((sign_d * 0.9 * a / 4, fs2 + f, th2 + ph))
                terms.append((sign_d * 0.9 * a / 4, fs2 - f, th2 - ph))
    if pilot is not None:
        terms.append((float(pilot), sf.PILOT_HZ * (1 + pilot_ppm * 1e-6), pilot_phase))
    t = np.arange(n, dtype=np.float64) / sf.FS
    phase = np.zeros(n)
    for a, f, ph in terms:
        phase += a * sf.DEV_HZ / f * (np.cos(ph) - np.cos(2 * np.pi * f * t + ph))
    x = amp * np.exp(1j * phase)
    if cnr_db is not None:
        rng = np.random.default_rng(seed)
        s = amp * 10 ** (-cnr_db / 20) / np.sqrt(2)
        x = x + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag), -32768, 32767)
    return out


@pytest.mark.parametrize("name", [k for k, v in fa.CASES.items() if v[0] is not None])
def test_source_is_bit_identical_without_rds(name):
    """every fm_args input: the source without `rds` gives the bytes the parent's source gave"""
    tx = {"amp": fa.AMP, **fa.CASES[name][0]}
    a = sf.fm_host(fa.N, **tx)
    assert a.tobytes() == _parent_fm_host(fa.N, **tx).tobytes() == sf.fm_host(fa.N, **tx, rds=None).tobytes() == fa.host(name).tobytes()
    assert type(sf.mpx_terms([(1000.0, 0.3)], [], 0.1, 0.0, 0.3, 75)) is list
    car = sf.fm_carrier(5000, fs=1488375.0, **{k: v for k, v in tx.items() if k not in ("amp", "cnr_db", "seed")})
    assert np.array_equal(car, np.exp(1j * sf.fm_phase(5000, sf.mpx_terms(tx.get("left", ()), tx.get("right", ()), tx.get("pilot", 0.1), tx.get("pilot_ppm", 0.0),
                                                                          tx.get("pilot_phase", 0.3), tx.get("preemph_us")), 1488375.0)))


def test_rds_groups_helper_and_simpson_error():
    g = sf.rds_groups(0x3AAB, "KEXP-FM ", text="Hi!", clock=(60310, 13, 37, -14), pty=5, tp=1)
    assert len(g) == 6 and all(a == 0x3AAB for a, _, _, _ in g)
    assert [b >> 12 for _, b, _, _ in g] == [0, 0, 0, 0, 2, 4] and all((b >> 5 & 31) == 5 and (b >> 10 & 1) for _, b, _, _ in g)
    assert bytes(v for _, _, _, d in g[:4] for v in (d >> 8, d & 255)) == b"KEXP-FM "
    dec = rm.Groups().push(np.tile(sf.rds_bits(g), 3))
    snap = dec.snapshot()
    assert snap["ps"] == b"KEXP-FM " and snap["rt"] == b"Hi!\r" and snap["clock"] == (60310, 13, 37, -14) and snap["pty"] == 5 and snap["tp"] == 1
    r = sf.RdsSignal(g, sf.PILOT_HZ, 0.3)
    a, b = r.phase_integral(4000, sf.FS, 8), r.phase_integral(4000, sf.FS, 32)
    assert np.max(np.abs(a - b)) * 2 * np.pi * 2000.0 < 1e-6                 # radians of carrier phase at dev_hz = 2 kHz
    assert eng.rds_callsign(0x3AAB) == "KQED" and eng.rds_callsign(0x54A8) == "WAAA" and eng.rds_callsign(0x994F) == "WZZZ"
    assert eng.rds_callsign(0x1000) == "KAAA" and eng.rds_callsign(0x0FFF) is None and eng.rds_callsign(0x9950) is None
    assert eng.rds_text(b"KEXP-FM ") == "KEXP-FM" and eng.rds_text(b"Hi!\r  ") == "Hi!" and eng.rds_text(b"a\xe9b") == "a�b"
    assert eng.rds_event_fields("ps", [0x3AAB], b"KEXP-FM ") == {"pi": 0x3AAB, "ps": "KEXP-FM", "raw": b"KEXP-FM "}


@pytest.mark.parametrize("name", list(ra.CASES))
def test_inputs_hold_what_they_are_named_for(name):
    ra.reference(name)


@pytest.mark.parametrize("name", list(ra.group_cases()))
def test_group_inputs_hold_what_they_are_named_for(name):
    ra.group_reference(name)


# ---------------------------------------------------------------------------------------------------------------- the CPU twin
def test_tables(be):
    rc.check_tables(be)


def test_matched_filter_timing_and_bits_through_the_stage_hook(be):
    rc.check_stage_signal(be)


@pytest.mark.parametrize("name", list(ra.CASES))
def test_session_equals_model(be, name):
    rc.check_session_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_with_different_schedules(be, k):
    rc.check_multi(be, k)


@pytest.mark.parametrize("plan", list(rc.chunk_plans(ra.N)))
def test_chunking_gives_identical_events(be, plan):
    rc.check_chunking(be, [plan])


def test_reset_and_enable_rules(be):
    rc.check_reset_and_enable(be)


def test_audio_is_untouched(be):
    rc.check_audio_untouched(be)


def test_launch_counts_without_and_with_rds(be):
    rc.check_launch_counts(be)


@pytest.mark.parametrize("name", list(ra.group_cases()))
def test_groups_equal_model(be, name):
    rc.check_groups_case(be, name)


def test_groups_stream_continues_in_the_next_call(be):
    rc.check_groups_in_pieces(be)


def test_groups_of_several_channels(be):
    rc.check_groups_many_channels(be)
