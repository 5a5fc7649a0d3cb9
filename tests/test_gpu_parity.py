"""`-m gpu`: parity of the real gfx950 library (through the C ABI, libnrsc5hip.so) against the CPU
oracle, the golden fixtures produced by the unmodified reference, and -- at full size -- against
size-independent properties (decoded frames == transmitted bits, batch == streaming, async == in-order)."""
import numpy as np
import pytest

from tests import common, engine_checks as ec
from nrsc5_amd import engine as eng, synth

pytestmark = pytest.mark.gpu


def test_gpu_lane_exchange_selftest(hip_lib):
    E = eng.Engine(max_streams=1, q15_capacity=2 * 71280, lib_path=hip_lib)
    assert E.stage_selftest() == 0
    E.close()


def test_gpu_halfband_exact(hip_lib, oracle):
    ec.check_halfband(hip_lib, oracle, n=200003)


def test_gpu_halfband_chunk_history(hip_lib, oracle):
    ec.check_halfband_streaming_history(hip_lib, oracle)


def test_gpu_fft2048(hip_lib, oracle):
    ec.check_fft(hip_lib, oracle, n=64)


def test_gpu_viterbi_exact_small(hip_lib, oracle):
    ec.check_viterbi(hip_lib, oracle, lens=(80, 2304, 4608), frames=8)


def test_gpu_viterbi_exact_p1_size(hip_lib, oracle):
    ec.check_viterbi(hip_lib, oracle, lens=(146176,), frames=3, structured=True)


def test_gpu_viterbi_roundtrip_many_frames(hip_lib):
    ec.check_viterbi_roundtrip(hip_lib, L=146176, frames=64)


@pytest.mark.parametrize("name", list(common.GOLDEN_CASES))
def test_gpu_golden_end_to_end(hip_lib, name, captures):
    ec.check_golden_end_to_end(hip_lib, name, captures)


@pytest.mark.parametrize("kw", [
    dict(n_frames=0, n_blocks=36, seed=21, cfo_hz=-212.0, offset=2501, snr_db=11.0),      # un-clamped soft-bit gain
    dict(n_frames=0, n_blocks=24, seed=22, cfo_hz=5000.0, offset=4000, snr_db=25.0),      # 14-bin CFO search
    dict(n_frames=0, n_blocks=20, seed=23, cfo_hz=0.0, offset=1234, snr_db=20.0),         # reference false-lock zone
    dict(n_frames=0, n_blocks=20, seed=24, cfo_hz=40.0, offset=10, snr_db=30.0, fmt="cs16"),
])
def test_gpu_oracle_end_to_end(hip_lib, oracle, kw):
    # In the reference's false-lock zone (MER < 0 dB, cber ~ 0.13) the Viterbi input is noise: +-1 LSB
    # soft-bit differences (libm / FFT rounding) then change decoded bits, in the reference as well when
    # its own FFT library changes.  Bit-exactness is asserted for decodable frames only.
    ec.check_oracle_end_to_end(hip_lib, oracle, kw, garbage_frames_ok=(kw["offset"] == 1234))


def test_gpu_noise_only_matches_oracle(hip_lib, oracle):
    """Unsynchronised worst case: acquisition + CFO search every block; the state trace must match."""
    rng = np.random.default_rng(5)
    iq = rng.integers(100, 156, size=2 * 1488375, dtype=np.uint8)
    exp, _, _ = oracle.run(iq)
    E = eng.Engine(max_streams=1, q15_capacity=1 << 20, lib_path=hip_lib)
    common.run_engine_streaming(E, 0, iq)
    got = eng.records_to_log(E, 0, E.drain(0))
    ints = ("state_before", "state_after", "samperr", "cfo", "keep", "cfo_wait")
    eb = [{k: v[k] for k in ints} for kk, v in exp if kk == "block"]
    gb = [{k: v[k] for k in ints} for kk, v in got if kk == "block"]
    assert eb == gb
    E.close()


def test_gpu_push_size_invariance(hip_lib, captures):
    cap = captures("fm_cu8_cfo-2400")
    logs = []
    for chunk in (4096, 32768, 1000004):
        E, recs, log = ec.run_capture(hip_lib, cap, chunk=chunk)
        logs.append(log)
        E.close()
    assert not common.compare_logs(logs[0], logs[1], rtol=0.0) and not common.compare_logs(logs[0], logs[2], rtol=0.0)


@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_batch_equals_streaming(hip_lib, p1_async):
    caps = [synth.fm_mp1_capture(0, seed=30 + k, cfo_hz=c, offset=o, snr_db=s, n_blocks=nb)
            for k, (c, o, s, nb) in enumerate([(50.0, 100, 18, 40), (-900.0, 3000, 15, 36), (300.0, 0, 25, 52), (-30.0, 1234, 20, 33),
                                               (120.0, 2222, 20, 17), (0.0, 4319, 12, 48)])]
    ec.check_batch_equals_streaming(hip_lib, caps, p1_async=p1_async)


def test_gpu_batch_equals_streaming_extended_modes(hip_lib):
    caps = [synth.fm_mp1_capture(0, seed=50 + k, cfo_hz=c, offset=o, snr_db=20, n_blocks=nb, mode=m)
            for k, (c, o, nb, m) in enumerate([(10.0, 100, 44, "MP11"), (-60.0, 3000, 41, "MP3"), (300.0, 0, 20, "MP1"), (0.0, 64, 40, "MP2")])]
    ec.check_batch_equals_streaming(hip_lib, caps, p1_async=True)


@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_interleaved_streams_and_subset_batches(hip_lib, p1_async):
    """Launch flags measured on one stream set must not leak into calls that list another (round-1 advisor finding)."""
    ec.check_interleaved_streams(hip_lib, p1_async=p1_async)


@pytest.mark.parametrize("p1_async,l2_feedback", [(True, False), (True, True), (False, False)])
def test_gpu_zero_copy_batch_equals_streaming(hip_lib, p1_async, l2_feedback):
    """Engine option batch_zero_copy: captures read in place (half-band fused into k_mixfft, acquisition window decimated on
    the fly) == the streaming seam, incl. CFO search, a falsely locking capture with replay, ragged lengths."""
    caps = [synth.fm_mp1_capture(0, seed=70 + k, cfo_hz=c, offset=o, snr_db=sn, n_blocks=nb)
            for k, (c, o, sn, nb) in enumerate([(40.0, 123, 18, 40), (-2300.0, 3001, 15, 24), (0.0, 1234, 20, 52), (280.0, 4319, 25, 36), (5000.0, 4000, 25, 24)])]
    ec.check_zero_copy_batch(hip_lib, caps, p1_async=p1_async, l2_feedback=l2_feedback)


def test_gpu_small_fifo_compaction(hip_lib, captures):
    ec.check_small_fifo_compaction(hip_lib, "fm_cu8_cfo137", captures)


def test_gpu_api_edges(hip_lib):
    ec.check_api_edges(hip_lib)


def test_gpu_large_push_into_minimum_fifo(hip_lib, oracle):
    ec.check_large_push_minimum_fifo(hip_lib, oracle)


def test_gpu_poisoned_results_are_rewritten(hip_lib):
    """nrsc5hip_debug_poison_results between two passes over one engine: the second pass's frames must be written by THAT pass
    (a skipped traceback would leave the 0xA5 pattern in the ring and its pinned host mirror)."""
    cap = synth.fm_mp1_capture(0, seed=62, cfo_hz=-50.0, offset=700, snr_db=22, n_blocks=36)
    stride = cap.iq.size + (-cap.iq.size) % 256
    buf = np.zeros((1, stride), dtype=np.uint8); buf[0, :cap.iq.size] = cap.iq
    E = eng.Engine(max_streams=1, q15_capacity=2 * 71280, record_capacity=512, p1_slots=8, p1_async=True, l2_feedback=True, batch_zero_copy=True, lib_path=hip_lib)
    dev = ec._to_device(E, buf)
    got = []
    for _ in range(2):
        E.reset_all()
        E.batch_append_cu8(dev, stride, [cap.iq.size - cap.iq.size % 4])
        E.batch_process(1)
        recs, counts, frames = E.batch_fetch_view(1)
        r = recs[0, :counts[0]]
        fr = [frames[0, int(x["p1_slot"])].copy() for x in r if int(x["flags"]) & eng.REC_P1]
        assert len(fr) >= 1 and not any((f == 0xA5A5A5A5).any() for f in fr)
        got.append(fr)
        E.poison_results()
        assert (frames[0] == 0xA5A5A5A5).all()                  # the view IS the pinned mirror
    truth = {np.packbits(f, bitorder="little").tobytes() for f in cap.p1_frames}
    # (the capture's timing offset makes the receiver lock falsely first: that frame is noise -- equal in both passes -- and fails its
    # header check; the frame after the re-acquisition is the transmitted one)
    assert len(got[0]) == len(got[1]) and all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))
    assert got[1][-1].tobytes() in truth
    ec._free_device(E, dev)
    E.close()


def test_gpu_cs16_batch(hip_lib, captures):
    ec.check_cs16_batch(hip_lib, captures)


def test_gpu_force_resync_feedback(hip_lib, oracle, captures):
    """L2 feedback seam (frame.c:535-540): dropping to NONE after the first P1 frame re-acquires like the oracle."""
    cap = captures("fm_cu8_cfo137")
    hits = []
    exp, _, _ = oracle.run(cap.iq, p1_hook=lambda bits: (hits.append(1) or len(hits) == 1))
    E = eng.Engine(max_streams=1, q15_capacity=1 << 20, lib_path=hip_lib)
    got, fired = [], False
    step = 32768
    for off in range(0, cap.iq.size, step):
        part = cap.iq[off:off + step]
        E.push_cu8(0, part[:part.size - part.size % 4])
        recs = E.drain(0)
        log = eng.records_to_log(E, 0, recs)
        if not fired and any(k == "frame" for k, _ in log):
            E.force_resync(0)
            fired = True
        got += log
    # the reference flips the state inside the frame's own block (its record ends in NONE); the engine applies
    # the host's request at the block boundary, so compare what drives the next block: state_before, timing, bc
    eb = [(v["state_before"], v["samperr"], v["bc"], v["cfo"]) for k, v in exp if k == "block"]
    gb = [(v["state_before"], v["samperr"], v["bc"], v["cfo"]) for k, v in got if k == "block"]
    assert eb == gb
    assert any(v["state_before"] == 0 for k, v in got[1:] if k == "block" and v is not got[0][1])
    ef = [v["bits"] for k, v in exp if k == "frame"]
    gf = [v["bits"] for k, v in got if k == "frame"]
    assert len(ef) == len(gf) and all(np.array_equal(a, b) for a, b in zip(ef, gf))
    E.close()


def test_gpu_full_size_truth_property(hip_lib):
    """BASELINE-size streams (20 s): every decoded P1 frame of a locked stream equals the transmitted
    bits and PIDS frames carry valid CRC-12 (size-independent property; the oracle is too slow here only
    in aggregate, so 3 streams)."""
    for seed, cfo, off in ((101, 211.0, 777), (102, -96.0, 3100), (103, 12.0, 2000)):
        cap = synth.fm_mp1_capture(14, seed=seed, cfo_hz=cfo, offset=off, snr_db=20.0)
        E = eng.Engine(max_streams=1, q15_capacity=cap.iq.size // 4 + 1024, record_capacity=512, p1_slots=16, p1_async=True, lib_path=hip_lib)
        dev = ec._to_device(E, cap.iq)
        E.batch_append_cu8(dev, 0, [cap.iq.size - cap.iq.size % 4])
        E.batch_process(1)
        recs, counts, frames = E.batch_fetch(1)
        r = recs[0, :counts[0]]
        p1r = r[(r["flags"] & eng.REC_P1) != 0]
        assert len(p1r) >= 13
        truth = np.packbits(np.array(cap.p1_frames, dtype=np.uint8), axis=1, bitorder="little")
        first = len(cap.p1_frames) - len(p1r)
        for j, rr in enumerate(p1r):
            assert np.array_equal(frames[0, int(rr["p1_slot"])].view(np.uint8), truth[first + j]), (seed, j)
        assert (p1r["ber"][1:] == 0).all()
        for rr in r[(r["flags"] & eng.REC_PIDS) != 0][-32:]:
            bits = eng.unpack_bits(rr["pids"], 80).reshape(-1, 8)[:, ::-1].reshape(-1)
            assert synth.crc12(bits) == int("".join(map(str, bits[68:80])), 2)
        ec._free_device(E, dev)
        E.close()


# ---- extended sidebands: MP2 / MP3 / MP11 (PX1 / PX2 -> interleaver IV -> P3 / P4) -------------------------------------
@pytest.mark.parametrize("mode,kw", [
    ("MP2", dict(n_blocks=52, seed=31, cfo_hz=20.0, offset=300, snr_db=25)),
    ("MP3", dict(n_blocks=54, seed=32, cfo_hz=-150.0, offset=500, snr_db=18, fmt="cs16")),
    ("MP11", dict(n_blocks=52, seed=33, cfo_hz=0.0, offset=64, snr_db=14)),
])
@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_extended_sidebands_oracle(hip_lib, oracle, mode, kw, p1_async):
    log = ec.check_oracle_end_to_end(hip_lib, oracle, dict(n_frames=0, mode=mode, **kw), p1_async=p1_async)
    assert sum(1 for k, v in log if k == "frame" and v["lc"] == 1) >= 2
    assert (mode != "MP11") or sum(1 for k, v in log if k == "frame" and v["lc"] == 2) >= 2


@pytest.mark.parametrize("mode", ["MP5", "MP6"])
@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_compatibility_modes_5_6_oracle(hip_lib, oracle, mode, p1_async):
    """PSMI 5 / 6 (sync.c:343-358 maps them to 14 partitions): equalised and measured like MP11, nothing routed to PX1 / PX2."""
    log = ec.check_oracle_end_to_end(hip_lib, oracle, dict(n_frames=0, n_blocks=50, seed=41, mode=mode, cfo_hz=35.0, offset=420, snr_db=22), p1_async=p1_async)
    assert not [v for k, v in log if k == "frame" and v["lc"] != 0] and any(k == "mer" for k, _ in log)
    assert sum(1 for k, v in log if k == "frame" and v["lc"] == 0) >= 1


# ---- AM (config 5) --------------------------------------------------------------------------------------------------
def test_gpu_am_viterbi_k9_exact(hip_lib, oracle):
    ec.check_viterbi_k9(hip_lib, oracle, lens=(80, 3750, 24000, 30000), frames=4)


def test_gpu_first_header_check(hip_lib, oracle):
    ec.check_first_header(hip_lib, oracle)


def test_gpu_am_viterbi_k9_segmented_exact(hip_lib, oracle):
    ec.check_viterbi_k9_segmented(hip_lib, oracle, lens=(3750, 24000, 30000), segments=(2, 3, 8))


def test_gpu_am_decimator_exact(hip_lib, oracle):
    ec.check_am_decimator(hip_lib, oracle)


@pytest.mark.parametrize("name", list(common.GOLDEN_AM_CASES))
def test_gpu_am_golden_end_to_end(hip_lib, name, captures):
    """Streaming seam in NRSC5_MODE_AM vs the trace of the unmodified reference: P1/P3/PIDS frames exact, floats 1e-4."""
    ec.check_am_golden_end_to_end(hip_lib, name, captures)


@pytest.mark.parametrize("kw", [
    dict(n_frames=10, seed=3, cfo_hz=3.0, offset=1234),
    dict(n_frames=9, seed=4, cfo_hz=200.0, offset=0),                 # integer carrier offset (acquire_cfo_adjust)
    dict(n_frames=9, seed=5, cfo_hz=-40.0, offset=9000, noise=2.0),
    dict(n_frames=2, seed=6, cfo_hz=10.0, offset=64 * 300 + 12, fmt="cu8"),
    dict(n_frames=9, seed=8, cfo_hz=-6.0, offset=2000, mode="MA3"),    # all-digital layout, 30000-bit P3 frames
])
def test_gpu_am_oracle_end_to_end(hip_lib, oracle, kw):
    ec.check_am_oracle_end_to_end(hip_lib, oracle, kw)


def test_gpu_am_batch_equals_streaming(hip_lib):
    ec.check_am_batch_equals_streaming(hip_lib, [dict(n_frames=10, seed=31, cfo_hz=5.0, offset=100),
                                                dict(n_frames=9, seed=32, cfo_hz=-20.0, offset=5000), dict(n_frames=3, seed=33)])
    ec.check_am_batch_equals_streaming(hip_lib, [dict(n_frames=2, seed=41, fmt="cu8"), dict(n_frames=1, seed=42, fmt="cu8", offset=3333)])


def test_gpu_am_window_pipeline_equals_in_order(hip_lib):
    ec.check_am_batch_equals_streaming(hip_lib, [dict(n_frames=14, seed=34, cfo_hz=7.0, offset=300), dict(n_frames=9, seed=35, offset=4000),
                                                dict(n_frames=12, seed=8, cfo_hz=-6.0, offset=2000, mode="MA3"),
                                                dict(n_frames=10, seed=36, cfo_hz=-3.0, offset=0)], p1_async=True)


# ---- the L2 -> L1 feedback on the device ------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(n_frames=0, n_blocks=40, seed=23, cfo_hz=0.0, offset=1234, snr_db=20.0),
    dict(n_frames=0, n_blocks=52, seed=15, cfo_hz=80.0, offset=2100, snr_db=22.0, mode="MP2"),
])
def test_gpu_l2_feedback_on_device_fm(hip_lib, oracle, kw):
    """RS(255,247) first-header check + drop to NONE inside the engine (in-order decode) == reference incl. its L2."""
    ec.check_l2_feedback(hip_lib, oracle, kw)


def test_gpu_l2_feedback_on_device_am(hip_lib, oracle):
    ec.check_l2_feedback(hip_lib, oracle, dict(n_frames=16, seed=9, cfo_hz=2.0, offset=500, burst=(8.3, 0.5, 40.0)), am=True)


@pytest.mark.parametrize("lag", [0, 2, 5])
def test_gpu_deferred_feedback_equals_reference(hip_lib, oracle, lag):
    """The benchmarked mode -- batch, window pipeline, on-device L2 feedback -- delivers the reference's log on false-lock
    captures: LOST_SYNC on the reference's block, re-acquisition, every frame (replay, k_replay.hip)."""
    ec.check_deferred_feedback_equals_reference(hip_lib, oracle, n_blocks=160, verdict_lag=lag,
                                                extra=((26, -120.0, 3333), (27, 250.0, 1234), (28, 0.0, 4000)))


@pytest.mark.parametrize("lag", [0, 2, 5])
def test_gpu_am_replay_equals_reference(hip_lib, oracle, lag):
    """AM batch, 8-step decode windows, L2 feedback on the device: the log equals the oracle driven by the restated
    frame_process decision however late the verdicts of the deferred decodes arrive (replay, k_rollback_am)."""
    ec.check_am_deferred_feedback_equals_reference(hip_lib, oracle, verdict_lag=lag)


def test_gpu_am_reduced_bandwidth(hip_lib, oracle):
    ec.check_am_reduced_bandwidth(hip_lib, oracle)


def test_gpu_mixed_batch_pipeline(hip_lib, oracle):
    ec.check_mixed_batch_pipeline(hip_lib, oracle, passes=3)


@pytest.mark.parametrize("case", ["cold_segments", "knobs"])
def test_gpu_am_replay_under_decode_knobs(hip_lib, oracle, case):
    """The window pipeline's own decode kernels (a) with warm-up and run-in switched off -- every P3 segment boundary takes the repair
    path -- and (b) with 3 segments on one decode stream confined to half the CUs at the lowest queue priority: the reference's log."""
    from nrsc5_amd import engine as eng
    if case == "cold_segments":
        ec.check_am_deferred_feedback_equals_reference(hip_lib, oracle, tunes=((eng.TUNE_AM_SEGMENTS, 5), (eng.TUNE_AM_WARM, 0)), expect_k9_repairs=True)
    else:
        ec.check_am_deferred_feedback_equals_reference(hip_lib, oracle, tunes=((eng.TUNE_AM_SEGMENTS, 3), (eng.TUNE_AM_DECODE_STREAMS, 1),
                                                                                 (eng.TUNE_DECODE_CUS, 16), (eng.TUNE_DECODE_PRIORITY, 1)))


def test_gpu_l2_feedback_deferred_recovers_false_locks(hip_lib):
    """Throughput mode: the feedback arrives when the deferred decode completes; falsely locked streams still re-acquire
    and then deliver the transmitted frames."""
    ec.check_deferred_feedback_recovers(hip_lib)


def test_gpu_l2_feedback_deferred_with_concurrent_hw_queues(hip_lib):
    """Same, in a fresh process with GPU_MAX_HW_QUEUES=8 (what bench.py runs with): the decode streams then really run
    beside the block-step chain, their verdicts arrive several windows late, and the verdicts of frames received before a
    re-acquisition must not knock down the new lock (lock-epoch tag on the request)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    code = "import sys; sys.path.insert(0, %r); from tests import engine_checks as ec; ec.check_deferred_feedback_recovers(%r); print('deferred-ok')" % (root, hip_lib)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "deferred-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_gpu_mode_switch_on_live_stream(hip_lib, reflib):
    ec.check_mode_switch(hip_lib, reflib)


def test_gpu_reset_of_a_used_stream_keeps_the_fir_windows(hip_lib, reflib):
    ec.check_reset_window_boundaries(hip_lib, reflib)
    ec.check_reset_keeps_fir_windows(hip_lib, reflib)
    ec.check_reset_keeps_fir_windows_am(hip_lib, reflib)


def test_gpu_pids_crc_flag(hip_lib, oracle):
    ec.check_pids_crc_flag(hip_lib, oracle)
    ec.check_pids_crc_flag(hip_lib, oracle, am=True)


def test_gpu_l2_index_every_branch(hip_lib, oracle):
    """k_l2_index (frame_push + frame_process's audio walk + CRC-8 of every packet) == the oracle's index, itself pinned
    against the unmodified reference's frame_push: all six frame lengths, every exit of the walk, bit-exact bytes."""
    ec.check_l2_index_stage(hip_lib, oracle)


@pytest.mark.parametrize("kw", [dict(am=False, mode="MP3"), dict(am=False, mode="MP11", p1_async=True), dict(am=True), dict(am=True, p1_async=True)])
def test_gpu_l2_index_end_to_end(hip_lib, oracle, kw):
    """IQ -> frames in HBM -> index, in-order and through the decode windows (FM P1 / P3 / P4, AM P1 / P3)."""
    ec.check_l2_index_end_to_end(hip_lib, oracle, **kw)


@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_l2_index_fused_into_decode(hip_lib, oracle, p1_async):
    """Engine option l2_index: index kernel on the decode stream behind each P1 traceback == post-pass == oracle."""
    ec.check_l2_index_fused(hip_lib, oracle, p1_async=p1_async)


def test_gpu_l2_index_vs_reference_golden(hip_lib):
    """Device index vs the calls the unmodified reference's frame_push made for the same frames (committed golden)."""
    ec.check_l2_index_vs_reference_golden(hip_lib)


def test_gpu_frame_push_indexed_with_device_index(hip_lib, reflib):
    """INTEGRATION.md's binding executed with the device's index inside the unmodified reference (needs oracle/_ref)."""
    ec.check_frame_push_indexed_with_device_index(hip_lib, reflib)


@pytest.mark.parametrize("p1_async", [False, True])
def test_gpu_hdc_consumer_equals_reference_events(hip_lib, reflib, p1_async):
    """device L2 index -> nrsc5hip_hdc_* (slim host state) == the unmodified reference's NRSC5_EVENT_HDC packets
    (program, count, flags, payload, order), incl. a capture with a false lock, LOST_SYNC and re-acquisition."""
    caps = [synth.fm_mp1_capture(4, seed=91, cfo_hz=35.0, offset=700, snr_db=22),
            synth.fm_mp1_capture(0, n_blocks=70, seed=23, cfo_hz=0.0, offset=1234, snr_db=20),
            synth.fm_mp1_capture(3, seed=52, cfo_hz=-40.0, offset=500, snr_db=25, mode="MP3")]
    assert ec.check_hdc_consumer(hip_lib, reflib, caps, p1_async=p1_async) >= 200


@pytest.mark.parametrize("am", [False, True])
def test_gpu_block_exact_pushes(hip_lib, oracle, am):
    ec.check_block_exact_pushes(hip_lib, oracle, am=am)


def test_gpu_viterbi_segmented_exact(hip_lib, oracle):
    ec.check_viterbi_segmented(hip_lib, oracle, lens=(2304, 4608, 146176), segments=(1, 2, 5, 16, 64))


def test_gpu_deferred_seam_equals_synchronous(hip_lib):
    """round 4's streaming seam on the device: block steps left in flight, read positions predicted under a sample-clock error, no
    P1 decode launches on blocks that cannot complete a frame, the drop-in's manual-step flow -- records and frames bit-identical
    to the synchronous seam, never a misprediction (tests/engine_checks.py: check_deferred_seam)"""
    ec.check_deferred_seam(hip_lib)


def test_gpu_host_capture_seam_equals_fifo_seam(hip_lib):
    """round 6's seam for FM cu8 (the session's bytes stay in a pinned capture the stream reads in place across PCIe) against the FIFO seam on the same pushes:
    records and frames bit-identical through buffer rebases, a cs16 push in mid-session, a reset of a used session, the batch entry point"""
    ec.check_host_capture_seam(hip_lib)


@pytest.mark.parametrize("syms", [4, 16])
def test_gpu_symbol_kernel_variants(hip_lib, syms):
    """k_mixfft's knob forms (4 symbols in a row per workgroup; 16 = two symbols side by side in a 256-lane workgroup): identical records"""
    caps = [synth.fm_mp1_capture(0, seed=71, cfo_hz=33.0, offset=400, snr_db=22, n_blocks=20), synth.fm_mp1_capture(0, seed=72, cfo_hz=-120.0, offset=1500, snr_db=20, n_blocks=20)]
    ec.check_zero_copy_batch(hip_lib, caps, p1_async=True, l2_feedback=False, mixfft_syms=syms)


def test_gpu_symbol_kernel_256_lanes(hip_lib, oracle, captures):
    """k_mixfft8 (knob 32), the 256-lane symbol kernel: FFT against float64 / the oracle, zero-copy batch == its own streaming form (rtol 0),
    golden traces of the unmodified reference end to end (frames exact, floats 1e-4)"""
    ec.check_fft(hip_lib, oracle, n=4, form=32)
    caps = [synth.fm_mp1_capture(0, seed=71, cfo_hz=33.0, offset=400, snr_db=22, n_blocks=20), synth.fm_mp1_capture(0, seed=72, cfo_hz=-120.0, offset=1500, snr_db=20, n_blocks=20)]
    ec.check_zero_copy_batch(hip_lib, caps, p1_async=True, l2_feedback=False, mixfft_syms=32, singles_tuned=True)
    for name in ("fm_cu8_cfo137", "fm_cu8_cfo-2400", "fm_cs16_cfo60", "fm_cu8_ppm60_host"):
        ec.check_golden_end_to_end(hip_lib, name, captures, tune=((ec.eng.TUNE_MIXFFT_SYMS, 32),))


@pytest.mark.parametrize("syms", [0, 32])
def test_gpu_zero_copy_batch_full_scale_captures(hip_lib, syms):
    """The production kernels' fused half-band at full scale: two captures loud enough to hit the rails -- rms_lsb 120: 3.8 % of the bytes
    are 0 or 255 (1.9 % each); rms_lsb 240: 28.5 % (14.4 % / 14.2 %), computed on the CPU; the usual 20 LSB capture has none -- through the
    zero-copy batch against the streaming seam (the integer decimator), record for record at rtol 0, in both forms of the symbol kernel
    (128 lanes; 32 = k_mixfft8, against its own streaming form).  Whatever the receiver makes of such captures: no frame is asserted."""
    caps = [synth.fm_mp1_capture(0, seed=91, cfo_hz=45.0, offset=611, snr_db=20, n_blocks=24, rms_lsb=120.0),
            synth.fm_mp1_capture(0, seed=92, cfo_hz=-310.0, offset=2750, snr_db=20, n_blocks=24, rms_lsb=240.0)]
    for cap, lo, hi in zip(caps, (0.03, 0.25), (0.05, 0.32)):
        assert lo < float(((cap.iq == 0) | (cap.iq == 255)).mean()) < hi
    ec.check_zero_copy_batch(hip_lib, caps, p1_async=True, l2_feedback=False, mixfft_syms=syms, rtol=0.0, singles_tuned=bool(syms))


def test_gpu_zero_copy_batch_full_range_noise(hip_lib):
    """One stream of uniform random bytes 0..255 (test_gpu_noise_only_matches_oracle's is 100..155): nothing ever locks, so every block goes
    through k_acq_decimate's half-band at full scale; zero-copy batch == streaming seam, record for record"""
    import types
    iq = np.random.default_rng(6).integers(0, 256, size=2 * 1488375, dtype=np.uint8)
    ec.check_zero_copy_batch(hip_lib, [types.SimpleNamespace(iq=iq)], p1_async=True, l2_feedback=False, rtol=0.0)


def test_gpu_traceback_variants(hip_lib):
    """single-path traceback == block-parallel traceback (records incl. the BER count, frames) on a capture with a noise frame"""
    ec.check_traceback_variants(hip_lib)


def test_gpu_exact_oscillator_first_block_is_the_references(hip_lib, reflib):
    """on the device the coarse angle goes through OCML's atan2f instead of glibc's (one ulp apart for ~16 % of arguments): bit-identical NCO
    state in at least half of the captures, never more than 1e-4 away"""
    ec.check_exact_oscillator_first_block(hip_lib, reflib, bit_exact_min=3, n=6)


def test_gpu_dataflow_bursts_equal_the_two_kernel_form(hip_lib):
    """k_flow on the MI355X: the block steps of a burst as ONE launch of symbol-pair and block-step work items that hand over to each other (write-through bins + a per-stream
    counter, agent-scope release / acquire around the stream state, parameter granules) -- every record and frame bit for bit as k_mixfft<1, 2> + k_sync<256> leave them, for
    24 streams (three per XCD list) of which two go through the CFO search and three carry a sample-clock error, with the replay on."""
    from nrsc5_amd import synth
    caps = []
    for k in range(24):
        if k % 8 == 3:
            caps.append(synth.fm_mp1_capture(**dict(common.IMPAIRED_FM_CASES["ppm+60"], n_blocks=48, seed=300 + k)))
        else:
            caps.append(synth.fm_mp1_capture(0, seed=300 + k, cfo_hz=(-2300.0 if k % 12 == 5 else 20.0 * k - 150.0), offset=(137 * k) % 4320, snr_db=18 + k % 5, n_blocks=40 + (k % 3) * 8))
    stats = ec.check_flow_bursts(hip_lib, caps, min_flow_steps=16)
    print("flow bursts / steps:", stats)
