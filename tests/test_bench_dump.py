"""bench.py --dump-outputs: the canonical float form of a launch's (desc, rec, heap) -- host logic only."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402
from pysignalduino_amd.runtime import DESC_DT, RES_DT, ST_OK, ST_RAISED  # noqa: E402


def _launch(n, seed, placement_seed):
    """A launch's host outputs for n messages (0-3 records each, 5 % raised): the contents depend on
    ``seed`` only, where each message's record block and payloads sit on ``placement_seed``."""
    rng = np.random.default_rng(seed)
    nrec = rng.integers(0, 4, n)
    status = np.where(rng.random(n) < 0.05, ST_RAISED, ST_OK).astype(np.uint8)
    nrec[status != ST_OK] = 0
    lens = [rng.integers(1, 40, k) for k in nrec]
    pays = [[rng.integers(0, 256, ln).astype(np.uint8) for ln in ls] for ls in lens]
    desc, rec, heap, off = np.zeros(n, DESC_DT), [], [np.zeros(0, np.uint8)], 0
    desc["status"] = status
    for m in np.random.default_rng(placement_seed).permutation(n):
        desc["rec_begin"][m], desc["n_rec"][m] = len(rec), nrec[m]
        for ln, p in zip(lens[m], pays[m]):
            rec.append((off, ln, 7 + m % 5, 4 * ln, m))
            heap.append(p)
            off += ln
    return desc, np.array(rec, RES_DT), np.concatenate(heap)


def _load(d):
    return {fn: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}


def test_dump_is_independent_of_record_placement(tmp_path):
    """Two launches with the same results placed differently (the kernels' atomic cursor) dump the same
    files; every array is float32 / float64 and the records follow message order."""
    dumps = []
    for i, ps in enumerate((3, 4)):
        f = {"MU": _launch(5000, 5, ps), "MC": _launch(3000, 6, ps + 10)}
        d = str(tmp_path / f"d{i}")
        nbytes = bench.dump_outputs(d, "", f)
        dumps.append(_load(d))
        assert nbytes == sum(a.nbytes for a in dumps[-1].values())
    assert sorted(dumps[0]) == [f"{k}_{p}.npy" for k in ("MC", "MU") for p in
                                ("desc", "msgs", "payload", "payload_msgs", "rec")]
    for fn, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64), fn
        assert np.array_equal(a, dumps[1][fn]), fn
    desc, rec, heap = f["MU"]
    d0 = dumps[0]
    assert np.array_equal(d0["MU_msgs.npy"], np.arange(5000))           # everything fits: every message
    assert np.array_equal(d0["MU_desc.npy"][:, 0], desc["n_rec"]) and np.array_equal(d0["MU_desc.npy"][:, 1], desc["status"])
    exp_rec, exp_pay = [], []
    for m in range(5000):
        for r in rec[desc["rec_begin"][m]: desc["rec_begin"][m] + desc["n_rec"][m]]:
            p = heap[r["payload_off"]: r["payload_off"] + r["payload_len"]].astype(np.int64)
            exp_rec.append((r["proto"], r["bit_length"], r["payload_len"],
                            int((p * (np.arange(len(p)) % 251 + 1)).sum()) % bench.CSUM_MOD))
            exp_pay.append(p)
    assert np.array_equal(d0["MU_rec.npy"], np.array(exp_rec, np.float32))
    assert np.array_equal(d0["MU_payload_msgs.npy"], np.arange(5000))   # ... and every payload byte
    assert np.array_equal(d0["MU_payload.npy"], np.concatenate(exp_pay).astype(np.float32))


def test_dump_samples_within_its_budget(tmp_path, monkeypatch):
    """Above the budget the dump is a seeded sample of messages: the same from run to run, within the
    budget (the message sample is sized from the mean record count, hence the 10 %), and each sampled
    message's payload bytes are the launch's."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100_000)
    f = {"MU": _launch(5000, 5, 3), "MC": _launch(3000, 6, 13)}
    a_bytes = bench.dump_outputs(str(tmp_path / "a"), "", f)
    bench.dump_outputs(str(tmp_path / "b"), "", {"MU": _launch(5000, 5, 8), "MC": _launch(3000, 6, 9)})
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a_bytes <= 1.1 * bench.DUMP_BUDGET
    for fn in a:
        assert np.array_equal(a[fn], b[fn]), fn
    msgs = a["MU_msgs.npy"].astype(np.int64)
    assert 0 < len(msgs) < 5000 and np.all(np.diff(msgs) > 0)
    pm = a["MU_payload_msgs.npy"].astype(np.int64)
    assert 0 < len(pm) < len(msgs) and np.all(np.isin(pm, msgs))
    desc, rec, heap = f["MU"]
    exp = [heap[r["payload_off"]: r["payload_off"] + r["payload_len"]]
           for m in pm for r in rec[desc["rec_begin"][m]: desc["rec_begin"][m] + desc["n_rec"][m]]]
    assert np.array_equal(a["MU_payload.npy"], np.concatenate(exp).astype(np.float32))


def test_dump_drops_records_outside_what_was_written(tmp_path):
    """A message whose record block or payload lies past what the launch wrote (an overflowed launch)
    dumps no records / no payload bytes instead of reading out of bounds."""
    desc, rec, heap = _launch(200, 7, 1)
    m = int(np.flatnonzero(desc["n_rec"] > 0)[0])
    desc["rec_begin"][m] = len(rec)               # block past the written records
    bench.dump_outputs(str(tmp_path), "", {"MS": (desc, rec, heap[: len(heap) // 2])})
    d = _load(str(tmp_path))
    assert d["MS_desc.npy"][m, 0] == 0
    assert len(d["MS_rec.npy"]) == int(d["MS_desc.npy"][:, 0].sum())
    assert len(d["MS_payload.npy"]) <= len(heap) // 2
