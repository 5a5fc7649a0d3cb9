"""`-m "not gpu"`: data services on the device (nrsc5hip_aas_*, csrc/k_aas.hip) on the CPU-emulated twin.  Three layers:
  the lists       tests/aas_args.py holds what it is named for, asserted on the model's output alone
  the model       tests/aas_model.py == the UNMODIFIED reference: its own output_aas_push, packet by packet, on every list on which the reference is well
                  defined (well-formed SIGs with a service, sizes up to 65 536, len >= 8; fragment events without their data)
  the device code nrsc5hip_stage_aas (the production kernel) == the model, event for event, counter for counter, SIG snapshot for snapshot: a list per call,
                  a packet per call, three streams in one call, reset, arena overflow, rejections; the chain frames -> k_psd -> k_aas with its byte bound and
                  a carousel sent three times; and the emulated engine end to end through nrsc5hip_aas_feed against the reference on the IQ
What only the device can show -- the generated code of the same kernel -- is tests/test_gpu_aas_stage.py's, which runs the same checks."""
import pytest

from nrsc5_amd import engine as eng
from tests import aas_args as aa, aas_checks as ac, aas_model as am


@pytest.fixture(scope="module")
def E(emu_lib):
    e = ac.make_engine(emu_lib)
    yield e
    e.close()


def _events(name, kind=None):
    return [ev for p in ac.expected(name)["packets"] for ev in p if kind is None or ev[0] == kind]


# ---- the lists and the model -------------------------------------------------------------------------------------------------------------------------
def test_files_holds_what_it_is_named_for():
    st, lst = ac.expected("files")["stats"], aa.files()
    assert st["before_sig"] == 2 and st["sig_packets"] == 2 and st["sig_parsed"] == 1 and st["not_in_sig"] == 1 and st["unknown_port"] == 4 and st["psd"] == 5
    assert st["stream"] == 2 and st["packet"] == 1 and st["unknown_type"] == 1 and st["lot_dropped"] == 1 and st["lot_too_large"] == 1
    lots = {ev[3][0]: ev for ev in _events("files", "lot")}
    assert sorted(lots) == [1, 2, 3, 4, 6] and st["lot_files"] == 5
    for lot, ev in lots.items():
        f = eng.aas_event_fields(*ev)
        assert f["data"] == lst["sent"][lot] and f["size"] in (1, 256, 257, 512, 300) and f["expiry"] == aa.EXPIRY
    assert lots[4][4][510:512] == lst["sent"][4][510:] == lst["sent"][4][510:511] + b"\0"     # the zero tail of a 255-byte fragment
    frag = _events("files", "lot_fragment")
    assert {ev[3][3] for ev in frag} >= {0, 1, 255, 256} and 257 not in {ev[3][3] for ev in frag}
    assert {ev[2] for ev in frag} >= {0, 1, 3, 4, 255} and 256 not in {ev[2] for ev in frag}
    assert st["lot_duplicates"] >= 3 and [ev[3][2] for ev in frag if ev[3][0] == 3] == [0, 1, 0]          # out of order, repeated
    per = ac.expected("files")["packets"]
    k = next(k for k, p in enumerate(lst["packets"]) if p[1] == 62)                                     # the header behind all fragments completes the file
    assert [ev[0] for ev in per[k]] == ["lot_header", "lot_fragment", "lot"] and per[k][1][3][2] == 1 and [ev[0] for ev in per[k + 1]] == ["lot_fragment"]
    sig = ac.expected("files")["sig"]
    assert [s["name"] for s in sig] == ["MPS", "Café data"] and [len(s["components"]) for s in sig] == [2, 4] and sig[0]["components"][0]["type"] == "audio"
    assert sorted(c["data_type"] for c in sig[1]["components"]) == [0, 1, 2, 3]


def test_headers_holds_what_it_is_named_for():
    st, per, lst = ac.expected("headers")["stats"], ac.expected("headers")["packets"], aa.headers()
    assert st["lot_dropped"] == 3 and st["lot_short_header"] == 2 and st["lot_resets"] == 2 and st["lot_headers"] == 5
    assert [ev[0] for ev in per[2]] == ["lot_fragment"] and per[3] == [] and per[4][0][3][2] == 0        # hdrlen 8; 15: stamped, and found again
    names = [ev[4] for ev in _events("headers", "lot_header")]
    assert names == [b"", lst["long_name"], b"ab", b"ab", b"ab"] and len(lst["long_name"]) == 231
    assert [len(p) for p in per[11:15]] == [3, 3, 3, 1]                                                # the NUL: starts over every time it is sent; "ab" is what was kept


def test_changes_holds_what_it_is_named_for():
    st, per = ac.expected("changes")["stats"], ac.expected("changes")["packets"]
    assert st["lot_resets"] == len(aa.CHANGES) == 9 and st["lot_files"] == 1 + 9 and st["lot_headers"] == 10
    assert [ev[0] for ev in per[3]] == ["lot_fragment"] and per[3][0][3][2] == 1                        # the same header again changes nothing
    hdr = [ev[3][1:8] + [ev[4]] for ev in _events("changes", "lot_header")]
    for a, b in zip(hdr, hdr[1:]):
        assert sum(x != y for x, y in zip(a, b)) == 1


def test_lru_and_pool_hold_what_they_are_named_for():
    st, lst = ac.expected("lru")["stats"], aa.lru()
    assert st["lru_evictions"] == 4 and st["pool_evictions"] == 0 and st["lot_resets"] == 1
    dup = {p[1]: ev[3][2] for p, evs in zip(lst["packets"], ac.expected("lru")["packets"]) for ev in evs if ev[0] == "lot_fragment"}
    assert (dup[22], dup[23], dup[37], dup[38]) == (0, 1, 1, 0)                                           # 101 was evicted, 100 not; of the two equals 103 went
    # without the touch the first file would have gone
    _, m = am.run([p for p in lst["packets"][:15] if p[1] != 20])
    assert not any(f is not None and f.lot == 100 for f in m.pool) and any(f is not None and f.lot == 101 for f in m.pool)
    st = ac.expected("pool")["stats"]
    assert st["pool_evictions"] == 3 and st["lru_evictions"] == 0
    assert [ev[3][2] for ev in _events("pool", "lot_fragment")] == [0, 0, 0, 0, 0, 0, 1, 0]


def test_big_aligned_and_short_hold_what_they_are_named_for():
    st = ac.expected("big")["stats"]
    lots = _events("big", "lot")
    assert st["lot_files"] == 1 and len(lots[0][4]) == 65536 + 7 and lots[0][4][:65536] == aa.big()["sent"][500] and st["lot_oversize"] == 2
    assert ac.expected("big")["packets"][-2][-1][0] == "lot"                                               # ... completed by the header on the last packet
    pads, at = set(), 0                                          # where the file bytes land in the arena when the list goes in one call
    for evs in ac.expected("aligned")["packets"]:
        for ev in evs:
            if ev[0] == "lot":
                pads.add((at + 48) % 16)
            at += 48 + (len(ev[4]) + 3) // 4 * 4
    assert pads >= {0, 4, 8, 12} and ac.expected("aligned")["stats"]["lot_files"] == 5
    st = ac.expected("short")["stats"]
    assert st["lot_dropped"] == 2 and st["lot_files"] == 1


@pytest.mark.parametrize("name", aa.SIG_CASES)
def test_sig_cases_hold_what_they_are_named_for(name):
    st, sig, per = ac.expected(name)["stats"], ac.expected(name)["sig"], ac.expected(name)["packets"]
    if name == "sig16":
        assert len(sig) == 16 and [s["number"] for s in sig] == list(range(200, 216)) and st["not_in_sig"] == 2 and st["stream"] == 1 and st["lot_packets"] == 1
    elif name == "sig9":
        assert len(sig) == 1 and len(sig[0]["components"]) == 8 and st["not_in_sig"] == 2 and st["lot_packets"] == 2
    elif name == "sigdup":
        assert [(s["number"], s["type"], s["name"]) for s in sig] == [(1, "audio", None), (5, "data", None)]
        assert [(c["id"], c["port"]) for c in sig[1]["components"]] == [(2, 0x1210), (3, 1)] and st["not_in_sig"] == 2 and st["stream"] == 1 and st["lot_packets"] == 1
    elif name == "sigstray":
        assert len(sig) == 1 and [c["port"] for c in sig[0]["components"]] == [aa.LOT_PORT] and st["not_in_sig"] == 3
    elif name == "sigtrunc":
        assert st["sig_truncated"] == 1 and [c["port"] for c in sig[0]["components"]] == [aa.LOT_PORT]
    elif name == "sigzero":
        assert st["sig_zero_length"] == 1 and [c["port"] for c in sig[0]["components"]] == [aa.LOT_PORT]
    else:
        assert st["sig_empty"] == 3 and st["sig_parsed"] == 4 and st["before_sig"] == 1 and [ev[4] for p in per[:4] for ev in p] == [b"", b"", b""]
        assert len(sig) == 2
    assert aa.get(name)["ref"] == (name in ("sig16", "sig9", "sigdup", "sigstray"))


@pytest.mark.parametrize("name", [n for n in aa.NAMES if aa.get(n)["ref"]] + ["carousel"])
def test_model_equals_the_reference(reflib, name):
    pk = aa.carousel(3)["packets"] if name == "carousel" else aa.get(name)["packets"]
    assert ac.model_vs_reference(reflib, pk) >= 4


def test_big_file_equals_the_reference(reflib):
    """the 64 KB file without the packets of the oversize one"""
    assert ac.model_vs_reference(reflib, [p for p in aa.big()["packets"] if p[0] != aa.LOT_PORT_B]) == 2 + 256 + 1


# ---- the device code -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aa.NAMES)
def test_list_in_one_call_equals_the_model(E, name):
    ac.check_list_in_one_call(E, name)


@pytest.mark.parametrize("name", ("files", "headers", "changes", "lru", "pool", "aligned", "signone"))
def test_one_packet_per_call_equals_the_model(E, name):
    ac.check_packet_per_call(E, name)


def test_fragment_events_only_with_the_flag(E):
    ac.check_fragment_flag_off(E)


def test_three_consumer_streams_in_one_call(E):
    ac.check_three_streams_in_one_call(E)


def test_reset_between_two_lists(E):
    ac.check_reset(E)


def test_arena_overflow_is_reported(E):
    ac.check_arena_overflow(E)


def test_rejections_leave_state_and_counters_untouched(emu_lib):
    ac.check_rejections(emu_lib)


def test_chain_behind_k_psd_three_streams(E):
    ac.check_chain(E)


def test_carousel_sent_three_times_moves_the_files_once(E):
    ac.check_carousel(E)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_feed_equals_the_reference(emu_lib, reflib):
    ac.check_feed_end_to_end(emu_lib, reflib)
