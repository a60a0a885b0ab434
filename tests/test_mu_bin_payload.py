"""Binary-dispatch MU payloads (finish_mu_lane in sdx_tile.h: '0' / '1' / 'F' digits, eight per step from
the packed bit words) against the C oracle, on a bank that is the shipped one plus copies of protocol 82
(Fernotron) with paddingbits 4 and 8, a three-character postamble and modulematches that walk the payload
byte by byte.  Frames of 100..128 bits with the float symbol at bit 0, 7, 8, 63, 64 and last, in batches
of 1, 65 and 129 through sdx_demod_pulses and sdx_demod_step; one all-Fernotron tile whose payloads
overflow the tile's LDS heap and go through the spilled writer.

Inputs and references: tests/mu_result_path_inputs.py (preconditions: tests/test_mu_result_path_inputs.py)."""
import functools

import numpy as np
import pytest

import mu_result_path_inputs as I

pytestmark = pytest.mark.gpu

ROUTES = ("pulses", "step")


@functools.lru_cache(None)
def _env():
    from pysignalduino_amd import bank as B, runtime
    bk = B.Bank(I.bin_protocols())
    return bk, runtime.Engine(bk, 0)


def _launch(route, pb):
    import torch
    from pysignalduino_amd import runtime
    bk, eng = _env()
    n = pb.n
    bd = eng.to_device_pulses(pb)
    out = eng.alloc_out(n, 16 * n + 1024, 2048 * n + 65536, eng.pulses_work_bytes(n))
    if route == "pulses":
        eng.launch_pulses(runtime.KIND_MU, bd, out, group=False)
    else:
        eng.launch_step(mu=(bd, out, None, None))
    torch.cuda.synchronize()
    assert int(out["cursor"][2].item()) == 0
    return eng.fetch(out), int(out["cursor"][3].item())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", I.BATCHES)
def test_binary_payloads_vs_c_oracle(n, route):
    frames, pb, ref = I.bin_frames()
    (desc, rec, heap), _ = _launch(route, pb.subset(np.arange(n)))
    assert I.compare(desc, rec, heap, ref[:n], _env()[0].mu_pids) == sum(len(e) for e in ref[:n] if isinstance(e, list))


@pytest.mark.parametrize("route", ROUTES)
def test_binary_payloads_through_the_spilled_writer(route):
    frames, pb, ref = I.bin_heavy()
    (desc, rec, heap), regions = _launch(route, pb)
    assert regions == 1   # the tile took a spill region
    assert I.compare(desc, rec, heap, ref, _env()[0].mu_pids) == sum(len(e) for e in ref)
