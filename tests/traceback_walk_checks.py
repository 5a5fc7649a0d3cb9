"""Checks of the single-path P1 traceback (k_p1_tbwalk / k_viterbi_frames_tbwalk + the verify-and-repair pass) shared by the device tests
(tests/test_gpu_traceback_walk.py) and their CPU-emulator twins (tests/test_traceback_walk_cpu.py).  The in-tree reference implementation is
the block-parallel traceback (TUNE_TRACEBACK_WALK = 0); the oracle's decoder is the outside one."""
import numpy as np

from nrsc5_amd import engine as eng, synth
from tests import common

P1_LEN = 146176
# frame lengths (multiples of 64, the smallest the entry takes) by the chunks they make, len / 64 + 1: a partial tile (6), a full tile (64),
# a second wave that holds one chunk (65) and two (66), a third wave (129); all three chunk phases (c % 3) occur from 6 chunks on
CHUNK_CASES = (6, 64, 65, 66, 129)
LENGTHS = tuple(64 * (n - 1) for n in CHUNK_CASES)


def stage_inputs(length, seed):
    """Three frames of soft values as the K=7 stage entry takes them (3 int8 per step, every sixth punctured): a random message encoded and
    sent at about 4 dB Eb/N0 (rate 2/5: Es/N0 = 0 dB, sigma = amplitude / sqrt 2), the same message at high SNR, and pure noise -- survivors
    merge slowly there, so the walk's speculation fails and the repair path runs."""
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, size=(1, length), dtype=np.uint8)
    coded = synth.conv_encode_k7(msg).reshape(3 * length).astype(np.float64) * 2 - 1
    amp = 32.0
    low = coded * amp + rng.normal(0, amp / np.sqrt(2.0), size=coded.shape)
    high = coded * amp + rng.normal(0, amp * 0.1, size=coded.shape)
    noise = rng.integers(-127, 128, size=coded.shape).astype(np.float64)
    soft = np.clip(np.rint(np.stack([low, high, noise])), -127, 127).astype(np.int8)
    soft[:, 5::6] = 0
    return msg[0], soft


def check_stage_lengths(lib, oracle, length, seed=71):
    msg, soft = stage_inputs(length, seed + length % 1009)
    got = {}
    for walk in (1, 0):
        E = eng.Engine(max_streams=1, q15_capacity=2 * 71280, lib_path=lib)
        if walk == 0:
            E.tune(eng.TUNE_TRACEBACK_WALK, 0)                  # (1 is the default: left untouched)
        got[walk] = E.stage_viterbi_k7(soft, length)
        if walk:
            stats = E.tb_stats()
        E.close()
    assert np.array_equal(got[1], got[0]), f"walk vs block-parallel traceback differ at len {length}"
    exp = np.stack([oracle.viterbi_k7(s) for s in soft])
    assert np.array_equal(got[1], exp), f"walk vs oracle differ at len {length}"
    assert np.array_equal(got[1][1], msg)                       # high SNR: the message itself
    assert stats[0] == 3 * (length // 64), stats                # every chunk boundary of the three frames was checked
    return stats


def check_engine_false_lock(lib, rewalk_max=None):
    """The false-lock capture of engine_checks.check_traceback_variants through the engine: records byte for byte (BER included) and frames
    equal between the walk and the block-parallel traceback, and the repair path ran."""
    cap = synth.fm_mp1_capture(0, seed=62, cfo_hz=-50.0, offset=700, snr_db=22, n_blocks=36)
    res = {}
    for walk in (0, 1):
        E = eng.Engine(max_streams=1, q15_capacity=1 << 20, record_capacity=256, p1_slots=8, lib_path=lib)
        E.tune(eng.TUNE_TRACEBACK_WALK, walk)
        common.run_engine_streaming(E, 0, cap.iq, chunk=32768 * 8)
        r = E.drain(0)
        frames = [E.p1_frame_bits(0, int(x["p1_slot"])).copy() for x in r if int(x["flags"]) & eng.REC_P1]
        res[walk] = (r.tobytes(), frames, E.tb_stats(), [float(x["ber"]) for x in r if int(x["flags"]) & eng.REC_P1])
        E.close()
    assert res[0][0] == res[1][0], "records differ between walk 0 and walk 1"
    assert len(res[0][1]) == len(res[1][1]) == 2 and all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert res[0][3] == res[1][3] and max(res[1][3]) > 0.1, res[1][3]      # the false lock's frame: Viterbi output on noise
    print("tb_stats", res[1][2], "ber", res[1][3])
    assert res[1][2][1] > 0, res[1][2]
    if rewalk_max is not None:
        assert res[1][2][1] <= rewalk_max, res[1][2]
    return res[1][2]
