"""Preconditions of tests/test_out_capacity.py's inputs, checked with the oracles alone (no GPU): the
capacity patterns of that module only mean what they say when these hold."""
import math

import numpy as np
import pytest

import out_capacity_inputs as I


def _raising(ref):
    return sum(1 for e in ref if not isinstance(e, list))


def test_mu_batch_has_raising_and_result_bearing_messages():
    pb, ref = I.mu_short()
    assert pb.n == 512 and int(np.diff(pb.offsets).max()) <= 256
    assert _raising(ref) >= 1
    assert sum(1 for e in ref if isinstance(e, list) and e) > pb.n // 2


# (input, messages per reservation unit, whether the launch reorders the messages first)
UNITS = [
    ("mu_short", lambda: I.mu_short()[1], 64, False),
    ("mu_grouped", lambda: I.mu_grouped()[1], 64, True),
    ("mu_long", lambda: I.mu_long()[1], 4, False),
    ("ms_tile64", lambda: I.ms_classes()[1], 64, False),
    ("ms_tile128", lambda: I.ms_classes()[1], 128, False),
    ("mc_block", lambda: I.mc_both()[2], 256, False),      # the <= 64-character launch flushes per 256-frame block;
    ("mc_wave", lambda: I.mc_both()[2], 64, False),        # the 65..128 one per wave: both within a block's frames
    ("mc_step", lambda: I.mc_step()[2], 256, False),
    ("mc_general", lambda: I.mc_general()[2], 1, False),
    ("general_mu", lambda: I.general_pulses("MU")[2], 1, False),
    ("general_ms", lambda: I.general_pulses("MS")[2], 1, False),
    ("mn_parser", lambda: I.mn_both()[1], 64, False),
    ("mn_method", lambda: I.mn_both()[2], 64, False),
]


@pytest.mark.parametrize("name,ref,unit,any_order", UNITS, ids=[u[0] for u in UNITS])
def test_largest_reservation_unit_needs_at_most_half_the_total(name, ref, unit, any_order):
    r, b, tr, tb = I.largest_unit(ref(), unit, any_order)
    assert I.half_fits(ref(), unit, any_order), (name, r, b, tr, tb)


def test_batches_reach_their_branches():
    pb, _ = I.mu_long()
    lens = np.diff(pb.offsets)
    assert pb.n == 64 and lens.min() > 256 and lens.max() <= 4096
    pb, ref = I.ms_classes()
    lens = np.diff(pb.offsets)
    assert (lens <= 128).sum() > 64 and (lens > 128).sum() > 64     # tiles of both length classes
    assert _raising(ref) + sum(1 for e in ref if isinstance(e, list) and e) > 0
    frames, mb, ref = I.mc_both()
    lens = np.diff(mb.offsets)
    assert (lens <= 64).sum() >= 1024 - 64 and ((lens > 64) & (lens <= 128)).sum() >= 256
    assert lens.max() <= 128
    frames, mb, _ = I.mc_general()
    assert np.diff(mb.offsets).min() > 128
    pb, _ = I.mu_grouped()
    assert pb.n >= I.runtime.GROUP_MIN
    for kind in ("MU", "MS"):
        msgs, gen, ref = I.general_pulses(kind)
        assert len(msgs) > 100 and sum(1 for e in ref if isinstance(e, list) and e) >= 4


def test_mn_modes_have_results_for_several_protocols():
    _, parser, method = I.mn_both()
    assert len({r[0] for e in parser for r in e}) >= 3
    assert sum(1 for e in method if e) > 16


def test_heavy_lines_overflow_the_first_attempt_but_not_the_fourth():
    """parse_lines_json starts an MU launch of k lines with 8k + 1024 records and grows x4 per attempt."""
    for min_rec in (16, 8):
        lines, sub, nr = I.heavy(min_rec)
        k, records = len(lines), int(nr.sum())
        assert k > 256 and int(np.diff(sub.offsets).max()) <= 256
        assert records > 8 * k + 1024, (min_rec, k, records)
        assert records <= 4 * (8 * k + 1024), (min_rec, k, records)


def test_heavy_lines_spill_more_tiles_than_the_workspace_has_regions():
    """A 64-message tile spills above 512 staged records; the batch API's workspace has max(16, tiles / 2)
    regions.  The 16-record subset stays within them, the 8-record one does not."""
    def spilling(nr):
        cuts = np.arange(0, len(nr), 64)
        return int((np.add.reduceat(nr, cuts) > 512).sum()), len(cuts)

    _, _, nr = I.heavy(16)
    over, tiles = spilling(nr)
    assert tiles <= 16                       # every tile can have a region
    _, _, nr = I.heavy(8)
    over, tiles = spilling(nr)
    assert over > max(16, math.ceil(len(nr) / 64) / 2), (over, tiles)
    # the stream's chunk capacity for the 16-record lines (8 C + 4096 records) is below their demand
    lines, _, nr16 = I.heavy(16)
    assert 8 * len(lines) + 4096 < int(nr16.sum())
