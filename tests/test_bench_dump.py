"""CPU: bench.py's --dump-outputs writer (dump_outputs) on synthetic records and frames -- the file set, the dtypes, the cleared bits past
a frame's length, the size bound -- and the split of the command line into a plain run and --full."""
import os

import numpy as np
import pytest

from nrsc5_amd import engine as eng


@pytest.fixture(scope="module")
def bench():
    import bench                          # imported here, not at collection: bench.py sets HIP environment defaults on import
    return bench


class _W:
    eng = eng

    def __init__(self, am):
        self.am = am

    def is_am(self, k):
        return self.am


def _batch(S, n, slots=6, seed=0):
    rng = np.random.default_rng(seed)
    recs = np.zeros((S, n), dtype=eng.RECORD_DTYPE)
    recs["p1_slot"] = np.arange(n) % slots
    recs["bc_decoded"] = np.arange(n) % 8
    recs["psmi"] = 2
    recs["flags"] = np.where(np.arange(n) % 4 == 0, eng.REC_P1 | eng.REC_P3, eng.REC_PROCESSED)
    recs["freq_offset"] = rng.standard_normal((S, n)).astype(np.float32)
    recs["pids"] = rng.integers(0, 2 ** 32, size=(S, n, 3), dtype=np.uint64).astype(np.uint32)
    counts = rng.integers(n // 2, n + 1, size=S).astype(np.int32)
    frames = rng.integers(0, 2 ** 32, size=(S, slots, eng.P1_WORDS), dtype=np.uint64).astype(np.uint32)
    return recs, counts, frames


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.mark.parametrize("am", [False, True])
def test_dump_files_dtypes_and_frames(bench, tmp_path, am):
    recs, counts, frames = _batch(24, 40)
    info = bench.dump_outputs(_W(am), recs, counts, frames, str(tmp_path))
    got = _load(str(tmp_path))
    assert set(got) == {"counts", "rec_streams", "frame_index", "frame_words"} | {"rec_" + n for n in eng.RECORD_DTYPE.names}
    assert info["files"] == len(got) and info["streams_with_records"] == 24
    for name, a in got.items():
        assert a.dtype == (np.float32 if name in ("rec_" + n for n in eng.RECORD_DTYPE.names if eng.RECORD_DTYPE[n].kind == "f") else np.float64), name
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["rec_streams"], np.arange(24))
    valid = np.concatenate([recs[k, :counts[k]] for k in range(24)])
    for n in eng.RECORD_DTYPE.names:
        assert np.array_equal(got["rec_" + n], valid[n]), n                # exact, 32-bit integers included
    # every announced frame of the sampled streams, its words exact and the bits past its length cleared
    sample = np.sort(np.random.default_rng(0).choice(24, size=bench.DUMP_FRAME_STREAMS, replace=False))
    per = 2 if am else 1
    assert got["frame_index"].shape == (sum(per * int((recs[k, :counts[k]]["flags"] & eng.REC_P1 != 0).sum()) for k in sample), 4)
    assert sorted(set(got["frame_index"][:, 0].astype(int))) == list(sample)
    for k, j, off, nw in got["frame_index"].astype(np.int64):
        r = recs[k, j]
        w = got["frame_words"][off:off + nw].astype(np.uint64)
        if not am:
            assert nw == eng.P1_WORDS and np.array_equal(w, frames[k, r["p1_slot"]])
        elif nw == (eng.AM_P1_BITS + 31) // 32:
            want = frames[k, r["p1_slot"], r["bc_decoded"] * eng.AM_P1_WORDS:][:nw].astype(np.uint64)
            assert np.array_equal(w[:-1], want[:-1]) and w[-1] == want[-1] & ((1 << (eng.AM_P1_BITS % 32)) - 1)
        else:
            assert nw == 30000 // 32 + 1
            want = frames[k, r["p1_slot"], eng.AM_P3_WORD0:][:nw].astype(np.uint64)
            assert np.array_equal(w[:-1], want[:-1]) and w[-1] == want[-1] & ((1 << (30000 % 32)) - 1)


def test_dump_stays_within_the_bound_and_samples_records(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 << 20)
    recs, counts, frames = _batch(64, 200)
    info = bench.dump_outputs(_W(False), recs, counts, frames, str(tmp_path))
    total = sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)))
    assert total <= 2 << 20 and info["bytes"] <= total
    got = _load(str(tmp_path))
    rows = got["rec_streams"].astype(int)
    assert 0 < rows.size < 64 and np.all(np.diff(rows) > 0)
    assert got["rec_flags"].size == int(counts[rows].sum())
    # the sample is fixed: the same call writes the same files
    d2 = tmp_path / "again"
    bench.dump_outputs(_W(False), recs, counts, frames, str(d2))
    again = _load(str(d2))
    assert all(np.array_equal(got[n], again[n]) for n in got)


def test_dump_per_rank_directories(bench, tmp_path):
    recs, counts, frames = _batch(8, 20)
    info = bench.dump_outputs(_W(False), recs, counts, frames, str(tmp_path), rank=1, world=2)
    assert info["dir"] == os.path.join(str(tmp_path), "rank1") and os.path.exists(os.path.join(info["dir"], "counts.npy"))


def test_plain_and_full_command_lines(bench):
    a = bench.parse(["--steps", "3", "--warmup", "1"])
    assert a.steps == 3 and a.warmup == 1 and not a.full and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"
