"""`-m "not gpu"`: SIS on the device (nrsc5hip_sis_*, csrc/k_sis.hip) on the CPU-emulated twin.  Three layers:
  the sets        tests/sis_args.py holds what it is named for, asserted on the model's / the reference's output alone
  the model       tests/sis_model.py == the UNMODIFIED reference: its public-API events on a 6-frame capture that carries the schedule, and its own
                  pids_frame_push on the random frames
  the device code nrsc5hip_stage_sis (the production kernel) == the model, event for event, counter for counter, snapshot for snapshot: a set per call, a
                  frame per call, pieces around the 64-frame chunk, three streams in one call, resets, arena overflow, rejections; and the emulated engine end
                  to end through nrsc5hip_sis_feed against the reference on the IQ
What only the device can show -- the generated code of the same kernel -- is tests/test_gpu_sis_stage.py's, which runs the same checks."""
import numpy as np
import pytest

from nrsc5_amd import engine as eng, synth
from tests import sis_args as sa, sis_checks as sc, sis_model as sm


@pytest.fixture(scope="module")
def E(emu_lib):
    e = sc.make_engine(emu_lib)
    yield e
    e.close()


# ---- the sets and the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1, 2))
def test_schedule_holds_what_it_is_named_for(variant):
    fr = sa.schedule(variant)
    per, m = sm.run(fr)
    st, kinds = m.stats, [ev[0] for f in per for ev in f]
    assert 90 <= len(fr) <= 130
    assert all(st["id%d" % k] >= 1 for k in range(11)) and st["id3"] >= 1                    # every message id, a reserved id 3
    assert st["unknown_id"] >= 2 and st["no_room"] >= 1 and st["llds"] >= 2                     # ids 11-15, a payload with no room, LLDS frames
    assert st["frames"] - st["crc_good"] >= len(fr) // 8                                        # about every 7th frame with a broken CRC
    assert not any(ev[3] == b"QQ" for f in per for ev in f)                                     # ... and none of them decoded
    logical = [synth._rev8(f) for f in fr]
    assert {int(b[1]) for b in logical} == {0, 1}                                               # both payload counts
    assert set(kinds) == set(eng.SIS_KINDS[1:])
    assert min(st["never_complete_message"], st["never_complete_slogan"], st["never_complete_alert"]) >= 1
    assert min(st["bad_checksum"], st["bad_crc7"], st["bad_cnt_crc"], st["bad_cnt_len"]) >= 1
    assert kinds.count("alert") == 2 and any(ev[0] == "alert" and ev[1][0] < 0 for f in per for ev in f)     # one valid alert, and its timeout
    assert kinds.count("audio_service") == 8 and st["id6"] + st["id10"] >= 26 and kinds.count("data_service") == 16   # 9 and 17 were sent
    assert kinds.count("leap_second") == 2 and kinds.count("exciter") == 1 and kinds.count("importer") == 1 and kinds.count("local_time") == 1
    msgs = [ev for f in per for ev in f if ev[0] == "station_message"]
    assert len(msgs) == 4 and any(ev[2] == 4 for ev in msgs) and "№" in sm.fields([e for e in msgs if e[2] == 4][0])[1]["message"]
    loc = [k for k, f in enumerate(per) for ev in f if ev[0] == "station_location"]
    assert len(loc) == 3                                                                        # longitude first: nothing until the latitude arrives
    # the long name / slogan rule in both directions
    slogans = [sm.fields(ev)[1]["slogan"] for f in per for ev in f if ev[0] == "station_slogan"]
    assert slogans == ([sa.STATIONS[0][0] + " long nm A", sa.STATIONS[0][4].decode()] if variant == 0 else [sa.STATIONS[variant][0] + " long nm A"])
    info = m.info()
    assert info["slogan"] == sa.STATIONS[variant][4].decode() and info["name"] == sa.STATIONS[variant][3].decode() + ("" if variant == 1 else "-FM")
    assert info["country"] == sa.STATIONS[variant][1] and info["fcc"] == sa.STATIONS[variant][2] and info["alert"] is None and info["location"] is not None
    assert len(info["audio_services"]) == 8 and len(info["data_services"]) == 16
    without = sa.schedule(variant, never_complete=False)
    s2 = sm.run(without)[1].stats
    assert len(without) <= 16 * sc.CAPTURE_FRAMES and s2["never_complete_message"] + s2["never_complete_slogan"] + s2["never_complete_alert"] == 0


@pytest.mark.parametrize("seed", sa.RANDOM_SEEDS)
def test_random_frames_are_valid_and_busy(seed):
    fr = sa.random_frames(seed)
    per, m = sm.run(fr)
    assert fr.shape == (256, 80) and m.stats["crc_good"] == 256 and m.stats["llds"] >= 10 and m.stats["events"] >= 30
    assert all(m.stats["id%d" % k] >= 3 for k in range(11)) and m.stats["unknown_id"] >= 30 and m.stats["no_room"] >= 5


def test_am_set_is_the_schedule_as_an_ma1_receiver_decodes_it():
    fr, sent = sa.am_frames(), sa.schedule(0, never_complete=False)
    assert len(fr) >= 80                                       # (the AM receiver delivers its first PIDS frame a few L1 frames into the capture)
    k = next(k for k in range(len(sent)) if np.array_equal(sent[k], fr[0]) and np.array_equal(sent[(k + 1) % len(sent)], fr[1]))
    assert all(np.array_equal(fr[j], sent[(k + j) % len(sent)]) for j in range(len(fr)))
    assert sc.expected("am")["stats"]["events"] >= 30


def test_model_equals_the_reference_events_on_the_capture(reflib):
    sc.model_vs_reference_capture(reflib)


@pytest.mark.parametrize("seed", sa.RANDOM_SEEDS)
def test_model_equals_the_reference_on_random_frames(reflib, seed):
    assert sc.model_vs_reference_frames(reflib, sa.random_frames(seed)) >= 30


@pytest.mark.parametrize("variant", (0, 1, 2))
def test_model_equals_the_reference_on_the_schedule_frames(reflib, variant):
    assert sc.model_vs_reference_frames(reflib, sa.schedule(variant, never_complete=False)) >= 40


def test_longest_items_complete_in_the_reference_and_in_the_model(reflib):
    """190, 95 and 381 bytes use every have_frame entry and complete; one frame more cannot be sent: the never-complete lengths start right behind"""
    fr = sa.longest()
    assert sc.model_vs_reference_frames(reflib, fr) == 3
    per, m = sm.run(fr)
    assert [(ev[0], len(ev[3])) for f in per for ev in f] == [("station_message", 190), ("station_slogan", 95), ("alert", 381)]
    assert [k for k, f in enumerate(per) if f] == [31, 47, 111] and m.stats["never_complete_message"] + m.stats["never_complete_slogan"] + m.stats["never_complete_alert"] == 0
    for item, counter in ((synth.sis_message(b"m" * 4, seq=0, length=191), "never_complete_message"), (synth.sis_slogan(b"s" * 5, length=96), "never_complete_slogan"),
                          (synth.sis_alert(synth.sis_alert_control(bytes(7)), b"", seq=0, length=382), "never_complete_alert")):
        m = sm.SisModel()
        assert m.push(synth.sis_frame([item[0]])) == [] and m.stats[counter] == 1


def test_text_conversion_is_the_reference_s():
    assert eng.sis_utf8(0, b"caf\xe9\0tail") == "café".encode() and eng.sis_utf8(4, "﻿№1".encode("utf-16-le")) == "№1".encode()
    assert eng.sis_utf8(4, b"\xfe\xff\x00A\x21\x16") == "A№".encode() and eng.sis_utf8(4, b"A\0B") == b"A" and eng.sis_utf8(4, b"") == b""
    assert eng.sis_utf8(1, b"abc") is None and eng.sis_text(7, b"") is None and eng.sis_text(0, b"") == ""


# ---- the device code -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sa.NAMES)
def test_set_in_one_call_equals_the_model(E, name):
    sc.check_set_in_one_call(E, name)


@pytest.mark.parametrize("name", ("schedule", "random1", "am"))
def test_one_frame_per_call_equals_the_model(E, name):
    sc.check_pieces(E, name, 1)


@pytest.mark.parametrize("piece", (63, 64, 65, 129))
def test_pieces_around_the_chunk_boundary(E, piece):
    for name in ("random3", "random4"):
        sc.check_pieces(E, name, piece)


def test_rewritten_lengths_of_displayed_items_stay_inside_the_snapshot(E):
    sc.check_rewritten_lengths(E)


def test_three_consumer_streams_in_one_call(E):
    sc.check_three_streams_in_one_call(E)


def test_reset_in_front_of_a_frame_mid_item_and_behind_the_last(E):
    sc.check_reset_at(E)


def test_sis_reset_mid_item(E):
    sc.check_reset_mid_item(E)


def test_arena_overflow_is_reported(E):
    sc.check_arena_overflow(E)


def test_rejections_leave_state_and_counters_untouched(emu_lib):
    sc.check_rejections(emu_lib)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_feed_in_record_pieces_equals_the_reference(emu_lib, reflib):
    sc.check_feed_end_to_end(emu_lib, reflib)


def test_am_records_feed(emu_lib):
    """an MA1 capture that carries the schedule through the emulated AM engine: nrsc5hip_sis_feed on its records == the model on the frames the records hold"""
    from tests import common
    cap = sa.am_capture()
    E = eng.Engine(max_streams=1, q15_capacity=cap.iq.size // 2 + 100000, record_capacity=256, p1_slots=8, am_enable=True, lib_path=emu_lib)
    C = eng.SisConsumer(E, 1)
    try:
        E.set_mode(0, eng.MODE_AM)
        common.run_engine_streaming(E, 0, cap.iq, chunk=32768)
        recs = E.drain(0)
        fl = recs["flags"]
        frames = np.stack([eng.unpack_bits(r["pids"], 80) for r in recs if int(r["flags"]) & eng.REC_PIDS])
        assert np.array_equal(frames, sa.am_frames())
        resets = [int(np.sum((fl[:k] & eng.REC_PIDS) != 0)) for k in np.nonzero(fl & eng.REC_TO_FINE)[0]]
        assert resets == [0]
        eng.feed_sis_batch(C, [0], [recs[:37]])
        eng.feed_sis_batch(C, [0], [recs[37:]])
        per = sc.expected("am")["frames"]
        n0 = int(np.sum((fl[:37] & eng.REC_PIDS) != 0))
        assert C.raw == sc.flat(per[:n0]) + sc.flat(per[n0:]) and sc.device_stats(C) == sc.expected("am")["stats"]
    finally:
        C.close()
        E.close()
