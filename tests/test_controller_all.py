"""BatchingParserTask(publish="json_all", rules=True) with the real SignalParser: per line, every
text of its reduced list to <base>/state/messages in order, then the line's _handle_as_command_response turn -- the
sequence of both kinds of calls is compared as ONE list with the per-line expectation built from the one-shot call
(parse_lines_json_all(dispatch=True), which test_dispatch_e2e.py holds against the reference's recorded lists)."""
import asyncio
import logging

import pytest

from pysignalduino_amd.controller import BatchingParserTask

from test_controller import Ctl, Pub, _drive
from test_dispatch_e2e import setup, sp  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


class LogPub(Pub):
    def __init__(self, events):
        super().__init__()
        self.events = events

    async def publish(self, *a):
        self.events.append(("pub",) + a)


class LogCtl(Ctl):
    """Publications and command-response turns in one list, in the order they happen."""

    def __init__(self, parser, pending=None):
        super().__init__(parser, callback=False)
        self.events = []
        self.mqtt_publisher = LogPub(self.events)
        self.logger = logging.getLogger("test_controller_all")
        if pending is not None:
            self._pending_responses = pending

    async def _handle_as_command_response(self, line):
        self.cmd.append(line)
        self.events.append(("cmd", line))


@pytest.fixture(scope="module")
def expected(setup, sp):   # noqa: F811
    s = setup
    lists = sp.parse_lines_json_all(s.lines, dispatch=True)
    assert [isinstance(x, s.ContractError) for x in lists] == s.ce
    ev = []
    for line, x in zip(s.lines, lists):
        if not isinstance(x, Exception):
            ev += [("pub", "t/v1/state/messages", t) for t in x]
        ev.append(("cmd", line))
    return ev


@pytest.mark.parametrize("stream,pending", [(True, None), (True, ["a pending command"]), (False, None), (False, ["a pending command"])])
def test_every_message_then_the_lines_turn(setup, sp, expected, stream, pending):   # noqa: F811
    s = setup
    assert all(s.lines)                                              # no empty line: every line has its turn
    ctl = LogCtl(sp, pending)
    task = BatchingParserTask(ctl, max_batch=512, publish="json_all", rules=True, stream=stream)
    asyncio.run(_drive(ctl, task, s.lines, chunk=300))
    assert ctl.events == expected
    assert task.lines == len(s.lines) and task.batches < len(s.lines) / 4
    if stream and pending is None:                                   # strictly more publications than publish="json"
        ctl2 = LogCtl(sp)
        asyncio.run(_drive(ctl2, BatchingParserTask(ctl2, max_batch=512, publish="json"), s.lines, chunk=300))
        n_all, n_one = sum(e[0] == "pub" for e in ctl.events), sum(e[0] == "pub" for e in ctl2.events)
        assert n_all > n_one + 300 and n_one > 1000
        assert [e for e in ctl2.events if e[0] == "cmd"] == [e for e in expected if e[0] == "cmd"]


@pytest.mark.parametrize("stream", [True, False])
def test_collapse_repeats_carries_the_run_across_micro_batches(setup, sp, stream):   # noqa: F811
    """Every decoding line twice: pairs straddle micro-batch ends.  Both values of ``stream`` publish what the mask of
    repeats.collapse_objects on the reduced lists leaves (test_stream_all.py's expectation)."""
    from pysignalduino_amd import repeats
    from test_dispatch_e2e import texts_of
    from test_stream_all import doubled
    s = setup
    idx, lines, objs = doubled(s)
    mask = repeats.collapse_objects(objs).tolist()
    exp = []
    for j, i in enumerate(idx):
        if not s.ce[i] and not mask[j]:
            exp += [("pub", "t/v1/state/messages", t) for t in texts_of(s.red[i])]
        exp.append(("cmd", lines[j]))
    ctl = LogCtl(sp)
    task = BatchingParserTask(ctl, max_batch=512, publish="json_all", rules=True, stream=stream, collapse_repeats=True)
    asyncio.run(_drive(ctl, task, lines, chunk=300))
    assert ctl.events == exp
    assert task.batches > 5
