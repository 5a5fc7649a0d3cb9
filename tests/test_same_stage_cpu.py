"""`-m "not gpu"`: SAME on the analog FM object (nrsc5hip_fm_same_*, nrsc5_amd/csrc/k_same.hip) on the CPU-emulated twin against the float64
restatement of its definition (tests/same_model.py); the checks are tests/same_checks.py, which tests/test_gpu_same_stage.py runs on gfx950.
The source and the helpers are pinned first: the burst's bits against a byte-by-byte expansion written here, the synthesiser's closed-form
phase integral against a numerical one, the source without `same` against the bytes it gave before the keyword existed, and same_fields."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth_fm as sf
from tests import fm_args as fa, same_args as sa, same_checks as sc, same_model as sm


@pytest.fixture(scope="module")
def be(emu_lib):
    return sc.Backend(emu_lib, gpu=False)


# ---------------------------------------------------------------------------------------------------------- the model and the source
def test_burst_bits_are_lsb_first_behind_sixteen_ab():
    bits = sf.same_bits("NNNN")
    assert bits.size == 8 * 20 and bits[:8].tolist() == [1, 1, 0, 1, 0, 1, 0, 1]                # 0xAB, the least significant bit first
    assert np.array_equal(bits[:128], np.tile(bits[:8], 16))
    assert bits[128:136].tolist() == [(ord("N") >> k) & 1 for k in range(8)]
    g = sm.Framer().push(np.concatenate([np.zeros(5, np.uint8), bits]))
    assert [(e["kind"], e["data"], e["first"], e["last"], e["v"][:3]) for e in g.events] == [("burst", b"NNNN", 133, 164, [sm.EOM, 1, 113])]


def test_same_signal_is_continuous_and_its_integral_closed():
    s = sf.SameSignal([(0.001, "NNNN")], level=0.3)
    fs = 8 * sf.FS
    t = np.arange(int(0.012 * fs)) / fs
    v = s.value(t)
    assert np.max(np.abs(np.diff(v))) < 0.3 * 2 * np.pi * 2100.0 / fs * 1.01                     # no step at a bit boundary: whole cycles per bit
    num = np.concatenate([[0.0], np.cumsum((v[1:] + v[:-1]) / 2) / fs])
    assert np.max(np.abs(num - s.phase_integral(t))) < 1e-9
    assert not s.value(np.array([0.0005, 0.5])).any() and not s.phase_integral(np.array([0.0005, 0.5])).any()
    # mark and space: four and three cycles per bit
    assert abs(4 * sf.SAME_BIT_HZ - 6250.0 / 3) < 1e-9 and abs(3 * sf.SAME_BIT_HZ - 1562.5) < 1e-9


@pytest.mark.parametrize("name", [k for k, v in fa.CASES.items() if v[0] is not None])
def test_source_is_bit_identical_without_same(name):
    """every fm_args input: the source without `same` gives the bytes it gave before"""
    tx = {"amp": fa.AMP, **fa.CASES[name][0]}
    assert sf.fm_host(fa.N, **tx).tobytes() == sf.fm_host(fa.N, **tx, same=None).tobytes() == fa.host(name).tobytes()
    assert type(sf.mpx_terms([(1000.0, 0.3)], [], 0.1, 0.0, 0.3, 75)) is list


def test_same_fields_and_lines():
    f = eng.same_fields("ZCZC-WXR-TOR-029095-029097+0030-1231405-KXYZ/FM -")
    assert f == {"originator": "WXR", "event": "TOR", "locations": ["029095", "029097"], "purge_minutes": 30, "day": 123, "hour": 14, "minute": 5,
                 "sender": "KXYZ/FM"}
    assert eng.same_fields(b"ZCZC-EAS-RWT-012345+0115-0010000-WABC    -")["purge_minutes"] == 75
    for bad in ("NNNN", "ZCZC-WXR-TOR-029095+0030-1231405-KXYZ/FM", "ZCZC-WXR-TOR+0030-1231405-KXYZ/FM -", "ZCZC-WXR-TOR-02909+0030-1231405-KXYZ/FM -", ""):
        assert eng.same_fields(bad) is None
    assert eng.same_line(sa.LONG) == "EAS WXR TOR 029095,029097 +0030 day 123 14:05 KXYZ/FM"
    assert eng.same_line("NNNN") == "EAS end of message"
    ev = eng.same_event_fields("message", [1, 2], sa.HEADER.encode())
    assert ev["kind"] == "header" and ev["bursts"] == 2 and ev["fields"]["locations"] == ["029095"] and ev["text"] == sa.HEADER
    assert eng.same_event_fields("burst", [2, 1, 113], b"NNNN") == {"text": "NNNN", "kind": "eom", "fields": None, "bursts": 1, "preamble_bits": 113}


@pytest.mark.parametrize("name", list(sa.CASES))
def test_inputs_hold_what_they_are_named_for(name):
    sa.reference(name)


@pytest.mark.parametrize("name", list(sa.frame_cases()))
def test_frame_inputs_hold_what_they_are_named_for(name):
    sa.frame_reference(name)


# ---------------------------------------------------------------------------------------------------------------- the CPU twin
def test_table_grid_and_latency(be):
    sc.check_table(be)


def test_tone_sums_timing_and_bits_through_the_stage_hook(be):
    sc.check_stage_signal(be)


@pytest.mark.parametrize("name", list(sa.CASES))
def test_session_equals_model(be, name):
    sc.check_session_case(be, name)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_channels_with_different_schedules(be, k):
    sc.check_multi(be, k)


@pytest.mark.parametrize("plan", list(sc.chunk_plans()))
def test_chunking_gives_identical_events(be, plan):
    sc.check_chunking(be, [plan])


def test_reset_and_enable_rules(be):
    sc.check_reset_and_enable(be)


def test_audio_and_d_are_untouched(be):
    sc.check_audio_untouched(be)


def test_launch_counts_without_and_with_same(be):
    sc.check_launch_counts(be)


@pytest.mark.parametrize("name", list(sa.frame_cases()))
def test_frames_equal_model(be, name):
    sc.check_frames_case(be, name)


def test_frames_stream_continues_in_the_next_call(be):
    sc.check_frames_in_pieces(be)


def test_frames_of_several_channels(be):
    sc.check_frames_many_channels(be)
