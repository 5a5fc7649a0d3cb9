"""`-m "not gpu"`: the PSD transport (nrsc5hip_psd_*, csrc/k_psd.hip) on the CPU-emulated twin.  Three layers:
  the sets        tests/psd_args.py holds what it is named for; the floors are asserted on the model's / the reference's output alone
  the model       tests/psd_model.py fed from the oracle's L2 index == the `l2aas` records of the UNMODIFIED reference, frame by frame
  the device code nrsc5hip_stage_psd (production index kernel + k_psd) == the model, packet for packet and counter for counter: a session per
                  call, a frame per call, three consumer streams in one call, a TO_FINE record and a reset with frames open, rejections; and the same through the
                  emulated engine end to end (sync and window pipeline, nrsc5hip_psd_feed in record pieces) against the reference on the IQ
What only the device can show -- the generated code of the same kernels -- is tests/test_gpu_psd_stage.py's, which runs the same checks."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth, wideband
from oracle import ref
from tests import common, psd_args as pa, psd_checks as pc, psd_model as pm


@pytest.fixture(scope="module")
def E(emu_lib):
    e = pc.make_engine(emu_lib)
    yield e
    e.close()


# ---- the sets and the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", pa.DENSE_SEEDS)
def test_dense_sessions_hold_what_they_are_named_for(E, oracle, seed):
    s = pa.dense(seed)
    d = pa.describe(s)
    assert set(pa.SPECIAL_SPANS) <= d["lens"]                   # 0, 1, 63, 64, 65, 128 and the PDU maximum
    assert set(pa.PROPS) <= d["hits"]                           # flags and escape pairs on the 64-byte step, on span ends and starts, across two frames
    assert len(s["pieces"][0][2]) == 5 and all(len(sp) == 12 for sp in s["spans"])
    assert {p for sp in s["spans"] for p, _ in sp} == set(pa.DENSE_PROGRAMS)
    idx, _ = oracle.l2_index(s["pieces"][0][2][0])
    assert idx["n_pdu"] == 12 and {(d_["prog_num"], d_["stream_id"]) for d_ in idx["pdus"]} >= {(2, 0), (2, 1)}
    raw = b"".join(s["streams"].values())
    assert b"\x7d\x7d\x7d" in raw and b"\x7e\x7e\x7e" in raw and b"\x7d\x7e" in raw      # runs of escapes, padding, a trailing escape
    st = pc.expected(oracle, E.lib, s["name"])["stats"]
    assert st["delivered"] >= 30 and min(st["bad_fcs"], st["wrong_protocol"], st["truncated_escape"]) >= 3, st
    sizes = [len(p[-1]) for fr in pc.expected(oracle, E.lib, s["name"])["frames"] for p in fr]
    assert max(sizes) >= 300 and min(sizes) < 80
    # frames shorter than protocol + port + seq + FCS with a good FCS: dropped as wrong protocol, where the reference hands a packet on
    model = pm.PsdModel()
    shorts = [f for f in (pa.hdlc(bytes([0x21]) + pa.SHORT_BODY[:n]) for n in range(4)) if f in raw]
    assert len(shorts) >= 2 and all(model.push_bytes(0, f) == [] for f in shorts) and model.stats["wrong_protocol"] == len(shorts)


@pytest.mark.parametrize("raw_len", pa.OVERFLOW_LENGTHS)
def test_overflow_set_delivers_exactly_what_the_rules_say(E, oracle, raw_len):
    s = pa.overflow(raw_len)
    exp = pc.expected(oracle, E.lib, s["name"])
    assert [p for fr in exp["frames"] for p in fr] == s["expect"]
    assert len(s["expect"]) == (2 if raw_len <= 8212 else 1) and exp["stats"]["overflows"] == s["expect_overflows"] == (0 if raw_len <= 8212 else 1)


def test_short_sessions_deliver_packets_on_every_form(E, oracle):
    for name in ("am", "p3_shared", "fixed"):
        assert pc.expected(oracle, E.lib, name)["stats"]["delivered"] >= 5, name
    shared = pa.p3_shared()
    assert [nbits for nbits, _, _ in shared["pieces"]] == [146176, 4608] * 4
    # a program's HDLC frames really run from a P1 frame into a P3 frame and back: fed alone, the P1 frames deliver fewer packets
    alone = pm.PsdModel()
    n = sum(len(alone.push_frame(*oracle.l2_index(b[0]))) for nbits, _, b in shared["pieces"] if nbits == 146176)
    assert n < pc.expected(oracle, E.lib, "p3_shared")["stats"]["delivered"] - 2


@pytest.mark.parametrize("name", pa.SESSION_NAMES)
def test_model_equals_the_reference_l2aas_records(E, oracle, reflib, name):
    n = pc.model_vs_reference(oracle, E.lib, reflib, name)
    if name.startswith("dense"):
        assert n >= 30


# ---- the device code -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pa.SESSION_NAMES)
def test_session_in_one_call_equals_the_model(E, oracle, name):
    pc.check_session_in_one_call(E, oracle, name)


@pytest.mark.parametrize("name", pa.SESSION_NAMES)
def test_one_frame_per_call_equals_the_model_and_the_frame_never_crosses(E, oracle, name):
    pc.check_frame_per_call(E, oracle, name)


def test_three_consumer_streams_in_one_call(E, oracle):
    pc.check_three_streams_in_one_call(E, oracle)


def test_to_fine_record_closes_open_frames_and_clears_the_fixed_data_state(E, oracle):
    pc.check_to_fine_reset(E, oracle)


def test_reset_with_frames_open(E, oracle):
    pc.check_reset_mid_frame(E, oracle)


def test_rejections_leave_state_and_counters_untouched(emu_lib, oracle):
    pc.check_rejections(emu_lib, oracle)


# ---- ID3 -----------------------------------------------------------------------------------------------------------------------------
def test_parse_id3_reads_the_generators_texts(E, oracle):
    seen = 0
    for name in ("dense1", "dense2", "am"):
        s = pa.session(name)
        got = {}
        for fr in pc.expected(oracle, E.lib, name)["frames"]:
            for program, port, seq, data in fr:
                if port in pa.PSD_PORTS:
                    tag = wideband.parse_id3(data)
                    assert tag is not None and pa.PSD_PORTS.index(port) == program
                    got.setdefault(program, []).append((tag["title"], tag["artist"]))
        for program, texts in got.items():
            # every intact ID3 packet of the stream, in order (the stream's tail may be cut inside a packet)
            assert texts == s["texts"][program][:len(texts)] and len(texts) >= len(s["texts"][program]) - 1
            seen += len(texts)
    assert seen >= 40
    tag = wideband.parse_id3(pa.id3_tag("Tïtle ~}", "Ärtist", album="Album", genre="Jazz", utf16=True))
    assert tag == {"title": "Tïtle ~}", "artist": "Ärtist", "album": "Album", "genre": "Jazz"}
    assert wideband.parse_id3(pa.id3_tag("cut\0tail", None)) == {"title": "cut"}
    good = pa.id3_tag("x", "y")
    for bad in (good[:9], b"ID3\x04" + good[4:], good[:5] + b"\x01" + good[6:], good[:-1], b""):     # the header checks of output.c:290-292
        assert wideband.parse_id3(bad) is None
    assert wideband.parse_id3(good + b"trailing bytes") == {"title": "x", "artist": "y"}


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_feed_in_record_pieces_equals_the_reference(emu_lib, reflib):
    """a 3-frame MP1 capture whose PDUs carry a PSD stream, through the emulated engine (sync and window pipeline, on-device L2 feedback);
    nrsc5hip_psd_feed in record pieces of 3 == the l2aas records of the unmodified reference on the same IQ"""
    rng = np.random.default_rng(5)
    stream = b"".join(pa.hdlc(pa.aas_payload(0x5100, k, pa.id3_tag("Title %d ~}" % k, "Artist %d" % k)), or_escape=k % 2 == 1) for k in range(8))
    cap = synth.fm_mp1_capture(3, seed=61, cfo_hz=25.0, offset=400, snr_db=22, psd_stream=stream)
    log, _, _ = reflib.run(cap.iq, taps=ref.TAP_L2)
    want = [v["data"] for k, v in log if k == "l2aas"]
    assert len(want) >= 3
    for p1_async in (False, True):
        E = eng.Engine(max_streams=1, q15_capacity=cap.iq.size // 4 + 200000, record_capacity=1024, p1_slots=16, lib_path=emu_lib, p1_async=p1_async, l2_feedback=True)
        common.run_engine_streaming(E, 0, cap.iq, chunk=32768 * 8)
        recs = E.drain(0)
        P = eng.PsdConsumer(E, 1)
        got = []
        for pos in range(0, len(recs), 3):
            moved = P.stats(0)["d2h_bytes"]
            new = eng.feed_psd_batch(E, P, [0], [recs[pos:pos + 3]])
            assert P.stats(0)["d2h_bytes"] - moved <= pc.bound(new)      # the frames stay on the device
            got += new
        assert [pm.packet_bytes(p) for p in got] == want, (p1_async, len(got), len(want))
        assert all(p[:2] == (0, 0) for p in got) and P.stats(0)["delivered"] == len(want)
        titles = [wideband.parse_id3(p[-1])["title"] for p in got]
        assert titles == ["Title %d ~}" % k for k in range(len(titles))]
        P.close()
        E.close()
