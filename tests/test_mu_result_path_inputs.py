"""Preconditions of tests/test_mu_bin_payload.py, from the C oracle alone
(no GPU): the inputs reach the code those tests are about, so a green GPU run cannot be vacuous."""
import mu_result_path_inputs as I
from pysignalduino_amd import bank as B


def test_bank_copies_compile_and_dispatch_binary():
    bk = B.Bank(I.bin_protocols())
    assert all(p in bk.mu_pids for p in I.BIN_IDS)
    assert len(bk.mu_pids) == len(B.Bank().mu_pids) + len(I.BIN_COPIES)


def test_every_bit_count_and_float_position_is_present():
    frames, pb, ref = I.bin_frames()
    assert pb.n == max(I.BATCHES) and len(ref) == pb.n
    plain, floats = set(), set()
    for f, e in zip(frames, ref):
        res = {r[0]: r for r in I.bin_results(e)}
        if "82" not in res:
            continue
        digits = res["82"][1][len(b"P82#"):].decode()
        assert digits == f and res["82"][2] == len(f)       # paddingbits 1: the frame as it is
        if "F" not in f:
            plain.add(len(f))
        for at in I.FLOAT_AT:
            if f[at] == "F" and f.count("F") == 1:
                floats.add((len(f), at))
    assert plain >= set(I.FRAME_BITS), sorted(set(I.FRAME_BITS) - plain)
    # every float position at every frame length (bit 63 / 64: either side of the packed words' boundary)
    assert floats >= {(nb, at) for nb in I.FRAME_BITS for at in I.FLOAT_AT}


def test_copies_pad_append_and_filter():
    frames, pb, ref = I.bin_frames()
    padded4 = padded8 = post = dropped = kept = walked_post = 0
    for f, e in zip(frames, ref):
        res = {r[0]: r for r in I.bin_results(e)}
        if "82" not in res:
            continue
        nb = len(f)
        assert res["82.4"][2] == -(-nb // 4) * 4 and res["82.8"][2] == -(-nb // 8) * 8
        assert res["82.4"][1] == b"P82#" + f.encode() + b"0" * (res["82.4"][2] - nb)
        assert res["82.8"][1] == b"P82#" + f.encode() + b"0" * (res["82.8"][2] - nb)
        padded4 += res["82.4"][2] > nb
        padded8 += res["82.8"][2] > nb
        assert res["82.9"][1] == b"P82#" + f.encode() + b"#Z9"
        post += 1
        if "F" in f[:8]:
            assert "82.7" not in res
            dropped += 1
        else:
            kept += "82.7" in res
        walked_post += "82.5" in res and res["82.5"][1].endswith(b"xyz")
    assert min(padded4, padded8, post, dropped, kept, walked_post) >= 10


def test_batches_have_binary_results_at_their_edges():
    _, _, ref = I.bin_frames()
    for n in I.BATCHES:   # the last message of every batch (message 64 and 128: the first of a new tile)
        assert I.bin_results(ref[0]) and I.bin_results(ref[n - 1])


def test_all_fernotron_tile_exceeds_the_lds_heap():
    frames, pb, ref = I.bin_heavy()
    assert pb.n == 64
    assert all(len(I.bin_results(e)) >= 2 for e in ref)                # two matches and more per message
    spans = sum((len(r[1]) + 7) & ~7 for e in ref for r in e)
    assert spans > I.PHEAP_MU
    binary = sum((len(r[1]) + 7) & ~7 for e in ref for r in I.bin_results(e))
    assert binary > 3 * I.PHEAP_MU                                      # most binary payloads are spilled
    assert spans <= I.PHEAP_MU + 40000                                  # within the spill region's 49,152 bytes
    assert sum("F" in r[1][4:].decode() for e in ref for r in I.bin_results(e)) >= 64
