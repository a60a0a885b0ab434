"""Batched parser loop for the controller.

The reference controller decodes one line per iteration (signalduino/controller.py:245-264):

    line = await self._raw_message_queue.get()
    decoded = await asyncio.to_thread(self.parser.parse_line, line)
    if decoded and self.message_callback: await self.message_callback(decoded[0])
    if self.mqtt_publisher and decoded:   await self.mqtt_publisher.publish(decoded[0])
    await self._handle_as_command_response(line)
    await asyncio.sleep(0.01)

:class:`BatchingParserTask` is a drop-in for ``SignalduinoController._parser_task``: it drains the
same queue into micro-batches (up to ``max_batch`` lines, waiting at most ``max_delay`` seconds
after the first one), decodes each batch with ONE ``SignalParser.parse_lines`` call in a worker
thread (one upload, one parse launch, one launch per demodulation kind, one read-back), then
performs the reference's per-line side effects in line order: the first decoded message only to
``message_callback`` and to the MQTT publisher, and ``_handle_as_command_response`` for every line.
A line outside the device contract (``ContractError`` in its slot) is logged and publishes
nothing -- like a line whose parser raised in the reference.

``publish="json"`` publishes the device-built texts instead (sdx_serialize_json):
``mqtt_publisher.client.publish(f"{base_topic}/state/messages", text)``, the call
MqttPublisher.publish makes (signalduino/mqtt.py:260-272) with the text its ``_message_to_json``
would build.  Its batches go through a pipelined :class:`~pysignalduino_amd.stream.LineStream`
(``stream=True``, the default): the upload, parse, demodulation and serialisation of batch k+1..k+3
run while the texts of batch k are published; when the queue runs dry for ``max_delay`` the stream
is drained, so a line's publication waits at most ``max_delay`` plus the GPU time of its batch.
``message_callback`` needs the objects, so it is only allowed with the default
``publish="objects"``.

Per-line overheads of the reference loop that have no observable effect are skipped exactly when
they have none: ``_handle_as_command_response(line)`` (controller.py:360-387) only matches pending
command responses and logs at DEBUG, so it is awaited for a line only while the controller has
pending responses or its logger is enabled for DEBUG (a controller without ``_pending_responses``
gets it for every line); an unbounded ``asyncio.Queue`` is drained in bulk.

``collapse_repeats=True`` drops consecutive equal telegrams (pysignalduino_amd/repeats.py: a line whose
first decoded message has the kind, protocol and payload of the previous decoding line's): such a line
causes no ``message_callback`` and no publication -- on the JSON path its text is never built -- while
``_handle_as_command_response`` still gets every line.  The run of equal lines continues across
micro-batches.  ``repeat_window=SECONDS`` (with ``collapse_repeats``) also ends a run once its last
published telegram is more than the window old, as FHEM dispatches (repeats.py): every line is stamped
with ``time.monotonic_ns() // 1000`` when it is taken from ``_raw_message_queue`` (``clock``: another
source of microseconds, for tests), and the stamps travel with the lines to the parser.

``routes`` (a routes.RouteTable or a list of (name, regex) pairs; with ``publish="json"``) matches every
decoded telegram's payload against an ordered client list on the device.
``route_topics=True`` publishes a routed text to ``<base_topic>/state/messages/<name>`` and an unrouted one
to ``<base_topic>/state/messages``; ``drop_unrouted=True`` publishes nothing for a telegram no route
matches (its text is never built) -- its line keeps its ``_handle_as_command_response`` turn, and it
starts and breaks runs of repeats as before.  The defaults publish exactly as without routes.
``route_match="any"``: of a line that demodulates to several messages, the first one that
some route matches is the telegram -- its text is published, to its client's topic with ``route_topics``.

``publish="json_all"`` publishes EVERY message of a line, as FHEM dispatches them: per line its
texts in order to ``<base_topic>/state/messages``, then the line's ``_handle_as_command_response`` turn under the
same check.  ``rules`` (None: every message; True or a dispatch.DispatchRules) reduces every line's list by FHEM's
dispatch rules first.  With ``stream=True`` the batches go through a ``json_all`` LineStream, with
``stream=False`` through one ``parse_lines_json_all`` call per micro-batch (with ``collapse_repeats`` through a
one-slot ``json_all`` LineStream drained per batch, which carries the run of repeats across micro-batches as the
``json`` path does).  It takes no routes and, like ``publish="json"``, no ``message_callback``.
"""
from __future__ import annotations

import asyncio
import collections
import logging
import time
from typing import Any, Callable, Deque, Dict, List, Optional


class BatchingParserTask:
    def __init__(self, controller: Any, max_batch: int = 4096, max_delay: float = 0.005, publish: str = "objects",
                 logger: Optional[logging.Logger] = None, stream: bool = True, lag: int = 3,
                 collapse_repeats: bool = False, repeat_window: Optional[float] = None,
                 clock: Optional[Callable[[], int]] = None, routes=None, drop_unrouted: bool = False,
                 route_topics: bool = False, route_match: str = "first", profiles=None, rules=None):
        if publish not in ("objects", "json", "json_all"):
            raise ValueError("publish must be 'objects', 'json' or 'json_all'")
        # every message of a line, reduced by the dispatch rules (§4o)
        self.all = publish == "json_all"
        from .dispatch import as_rules
        self.rules = as_rules(rules)
        if self.rules is not None and not self.all:
            raise ValueError("rules need publish='json_all'")
        if self.all and (routes is not None or drop_unrouted or route_topics or route_match != "first"):
            raise ValueError("publish='json_all' takes no routes")
        # receiver profiles: a controller reads ONE receiver, so the table has one source
        from .profiles import as_profiles
        self.profiles = as_profiles(profiles)
        if self.profiles is not None and self.profiles.n_sources != 1:
            raise ValueError("a controller reads one receiver: profiles with one source (a Profile)")
        # payload routes: the texts' routes come from the device, so they need publish='json'
        from .routes import as_table
        self.routes = as_table(routes)
        if route_match not in ("first", "any"):
            raise ValueError(f"route_match must be 'first' or 'any', not {route_match!r}")
        if route_match == "any" and self.routes is None:
            raise ValueError("route_match='any' needs routes")
        self.route_match = route_match
        self.drop_unrouted, self.route_topics = bool(drop_unrouted), bool(route_topics)
        if (self.drop_unrouted or self.route_topics) and self.routes is None:
            raise ValueError("drop_unrouted / route_topics need routes")
        if self.routes is not None and publish != "json":
            raise ValueError("routes need publish='json'")
        if publish != "objects" and getattr(controller, "message_callback", None):
            raise ValueError(f"publish='{publish}' produces texts only; message_callback needs publish='objects'")
        if max_batch < 1:
            raise ValueError("max_batch must be >= 1")
        self.c = controller
        self.max_batch = max_batch
        self.max_delay = max_delay
        self.publish = publish
        self.logger = logger or getattr(controller, "logger", None) or logging.getLogger(__name__)
        self.batches = 0
        self.lines = 0
        self.use_stream = stream and publish != "objects"
        self.lag = lag
        self._stream = None
        self.collapse = bool(collapse_repeats)
        self._last_key = None     # publish='objects': the key of the last decoding line (repeats.objects_key)
        from .repeats import window_to_us
        self.window_us = window_to_us(repeat_window)
        if self.window_us is not None and not self.collapse:
            raise ValueError("repeat_window needs collapse_repeats=True")
        self.clock = clock or (lambda: time.monotonic_ns() // 1000)
        self._stamps: List[int] = []          # repeat_window: the arrival times of _next_batch's lines
        self._carry = [None, 0, None]         # repeat_window, publish='objects': K, T, the last line's time

    def install(self) -> "BatchingParserTask":
        """Replace the controller's per-line loop (the attribute its run() schedules)."""
        self.c._parser_task = self.run
        return self

    def _take(self, q: asyncio.Queue, batch: List[Any]) -> None:
        """Move up to max_batch - len(batch) queued lines into batch without waiting: an unbounded
        asyncio.Queue is drained straight from its deque (no putter can be waiting on it, and the
        reference loop never calls task_done), any other queue with get_nowait()."""
        k = self.max_batch - len(batch)
        dq = getattr(q, "_queue", None)
        if type(q) is asyncio.Queue and q.maxsize <= 0 and isinstance(dq, collections.deque):
            if k >= len(dq):          # the whole queue fits: one bulk move
                batch.extend(dq)
                dq.clear()
            elif 8 * k >= len(dq):    # most of it: copy out and put the rest back (C-level copies)
                rest = list(dq)
                dq.clear()
                batch.extend(rest[:k])
                dq.extend(rest[k:])
            else:
                pop = dq.popleft
                batch.extend([pop() for _ in range(k)])
            return
        for _ in range(k):
            try:
                batch.append(q.get_nowait())
            except asyncio.QueueEmpty:
                return

    async def _next_batch(self, first_timeout: Optional[float] = None) -> List[Any]:
        """Up to max_batch lines, waiting at most max_delay after the first; with ``first_timeout``
        [] when no line arrives within it."""
        q: asyncio.Queue = self.c._raw_message_queue
        timed = self.window_us is not None
        if first_timeout is None:
            batch = [await q.get()]
        else:
            try:
                batch = [await asyncio.wait_for(q.get(), first_timeout)]
            except asyncio.TimeoutError:
                return []
        if timed:
            self._stamps = [self.clock()]
        loop = asyncio.get_running_loop()
        deadline = loop.time() + self.max_delay
        while len(batch) < self.max_batch:
            n0 = len(batch)
            self._take(q, batch)
            if timed and len(batch) > len(self._stamps):   # taken together: one reading of the clock
                self._stamps += [self.clock()] * (len(batch) - len(self._stamps))
            if len(batch) > n0:
                continue
            remaining = deadline - loop.time()
            if remaining <= 0:
                break
            try:
                batch.append(await asyncio.wait_for(q.get(), remaining))
            except asyncio.TimeoutError:
                break
            if timed:
                self._stamps.append(self.clock())
        return batch

    def _times_of(self, batch: List[Any]) -> Optional[List[int]]:
        """The stamps of the batch's non-empty lines (None without a window)."""
        if self.window_us is None:
            return None
        return [t for ln, t in zip(batch, self._stamps) if ln]

    def _topic(self, base: str, route: int) -> str:
        """<base>/state/messages, with route_topics <base>/state/messages/<name> for a routed text."""
        if self.route_topics and route >= 0:
            return f"{base}/state/messages/{self.routes.names[route]}"
        return f"{base}/state/messages"

    def _route_kw(self) -> dict:
        kw = {} if self.profiles is None else {"profiles": self.profiles}   # without profiles the calls are as before
        if self.routes is None:
            return kw
        kw.update(routes=self.routes, drop_unrouted=self.drop_unrouted)
        if self.route_match != "first":   # "first" calls exactly as before
            kw["route_match"] = self.route_match
        return kw

    def _profile_kw(self) -> dict:
        return {} if self.profiles is None else {"profiles": self.profiles}

    @staticmethod
    def _routed_items(r) -> List[Any]:
        """A routed chunk's items: (line, (route, text)), a ContractError as it is."""
        return [(i, (route, x) if isinstance(x, str) else x) for i, route, x in r.items_routed()]

    async def _publish_json(self, text: Any) -> None:
        route = -1
        if isinstance(text, tuple):   # routes: (route, text)
            route, text = text
        pub = self.c.mqtt_publisher
        client = getattr(pub, "client", None)
        if not client:
            self.logger.warning("Attempted to publish without an active MQTT client.")
            return
        try:
            await client.publish(self._topic(pub.base_topic, route), text)
        except Exception:  # noqa: BLE001  (mqtt.py:271-272)
            self.logger.error("Failed to publish message", exc_info=True)

    def _cmd_check(self) -> bool:
        """Whether _handle_as_command_response can have an effect now (see the module docstring)."""
        c = self.c
        pend = getattr(c, "_pending_responses", None)
        if pend is None:
            return True
        lg = getattr(c, "logger", None)
        return bool(pend) or (lg is not None and lg.isEnabledFor(logging.DEBUG))

    async def _publish_items(self, lines: List[Any], items: List[Any]) -> None:
        """The reference's per-line effects for one chunk, from its sparse results ``items`` =
        [(line index, text or exception)] in line order: per line, the publication of its text, then
        its _handle_as_command_response turn if _cmd_check() holds at that point.  The check can only
        change across an await, so after a false check the lines up to the next result (nothing is
        awaited for them) are skipped without re-checking."""
        c = self.c
        pend = getattr(c, "_pending_responses", None)
        if pend is None:        # no pending-response list: every line gets its turn
            res_at = dict(items)
            for i, line in enumerate(lines):
                res = res_at.get(i)
                if res is not None:
                    for x in (res if isinstance(res, list) else [res]):   # json_all: the line's texts in order
                        await self._publish_one(line, x)
                await c._handle_as_command_response(line)
            return
        lg = getattr(c, "logger", None)
        dbg = lg.isEnabledFor if lg is not None else (lambda _lv: False)
        handle = c._handle_as_command_response
        pub = c.mqtt_publisher
        client = getattr(pub, "client", None) if pub else None
        topic = f"{pub.base_topic}/state/messages" if client else None
        log = self.logger
        D = logging.DEBUG
        quiet = not (pend or dbg(D))    # the check for the next line
        j = 0                           # the next line whose turn is still open
        for i, res in items + [(len(lines), None)]:
            while not quiet and j < i:  # lines without a result: their command-response turns
                await handle(lines[j])
                j += 1
                quiet = not (pend or dbg(D))
            if i == len(lines):
                break
            if isinstance(res, Exception):   # parse_line raised for this line
                log.error("Parser error for line %r: %s", lines[i], res)
            elif pub:
                if not client:
                    log.warning("Attempted to publish without an active MQTT client.")
                else:
                    for x in (res if isinstance(res, list) else [res]):   # json_all: the line's texts in order
                        try:
                            if isinstance(x, tuple):   # routes: (route, text)
                                await client.publish(self._topic(pub.base_topic, x[0]), x[1])
                            else:
                                await client.publish(topic, x)
                        except Exception:  # noqa: BLE001  (mqtt.py:271-272)
                            log.error("Failed to publish message", exc_info=True)
                    quiet = not (pend or dbg(D))
            if not quiet:
                await handle(lines[i])
                quiet = not (pend or dbg(D))
            j = i + 1

    async def _publish_one(self, line: Any, res: Any) -> None:
        if isinstance(res, Exception):   # parse_line raised for this line
            self.logger.error("Parser error for line %r: %s", line, res)
        elif self.c.mqtt_publisher:
            await self._publish_json(res)

    async def _run_stream(self) -> None:
        """publish='json' through a pipelined LineStream (chunks = micro-batches).  Every line taken
        off the queue is published, as in the reference loop: when the stop event is set or an error
        ends the loop, the chunks still in flight are drained and published.  submit,
        poll and drain run in worker threads (poll may launch kernels and run the host parse of
        lines the device hands back), never on the event loop."""
        c = self.c
        if self._stream is None:
            kw = {"collapse_repeats": True} if self.collapse else {}
            if self.window_us is not None:
                kw["repeat_window"] = self.window_us / 1e6
            if self.rules is not None:
                kw["rules"] = self.rules
            self._stream = c.parser.stream(chunk_lines=self.max_batch, output="json_all" if self.all else "json",
                                           lag=self.lag, **kw, **self._route_kw())
        ls = self._stream
        # chunk id -> its lines: results are matched to their lines by id, never by position, so a
        # publication that fails part-way through a chunk cannot shift later chunks onto the wrong lines
        # (ADVICE r05); ``ready`` holds the finished chunks not yet published (a failure leaves the rest
        # of its poll's chunks there, and the exit drain publishes them)
        pending: Dict[int, List[Any]] = {}
        ready: Deque[Any] = collections.deque()

        async def publish(done):
            ready.extend(done)
            while ready:
                r = ready.popleft()
                blines = pending.pop(r.id)
                items = (r.items_all() if self.all else self._routed_items(r) if self.routes is not None else
                         r.items() if hasattr(r, "items") else [(i, t) for i, t in enumerate(r.texts()) if t is not None])
                self.lines += len(blines)
                await self._publish_items(blines, items)

        while not c._stop_event.is_set():
            try:
                batch = await self._next_batch(self.max_delay if pending else None)
                lines = list(filter(None, batch))
                if lines:
                    times = self._times_of(batch)
                    pending[await asyncio.to_thread(ls.submit, lines, **({} if times is None else {"times": times}))] = lines
                    self.batches += 1
                    done = await asyncio.to_thread(ls.poll)
                elif pending:           # the queue ran dry: publish everything in flight
                    done = await asyncio.to_thread(ls.drain)
                else:
                    done = []
                await publish(done)
                await asyncio.sleep(0)
            except asyncio.CancelledError:
                raise
            except Exception as e:  # noqa: BLE001  (controller.py:262-264)
                self.logger.error(f"Parser task error: {e}")
                break
        if pending:                     # stopped or failed with chunks in flight: publish them
            n = sum(len(b) for b in pending.values())
            try:
                await publish(await asyncio.to_thread(ls.drain))
            except asyncio.CancelledError:
                raise
            except Exception as e:  # noqa: BLE001
                self.logger.error(f"Parser task error while draining {n} in-flight lines: {e}")

    def _parse_collapsed(self, lines: List[Any], times: Optional[List[int]] = None) -> List[Any]:
        """One micro-batch with the repeats dropped, the run continuing from the previous batch: texts
        through a LineStream drained per batch (its state carries the last key on the device), objects
        through parse_lines with the last key kept here.  ``times`` (repeat_window): the lines' stamps;
        the objects are then marked here, from the carried (K, T) on (repeats.collapse_objects)."""
        p = self.c.parser
        if self.publish == "json":
            if self._stream is None:
                kw = {} if times is None else {"repeat_window": self.window_us / 1e6}
                self._stream = p.stream(chunk_lines=self.max_batch, output="json", lag=1, collapse_repeats=True, **kw,
                                        **self._route_kw())
            self._stream.submit(lines, **({} if times is None else {"times": times}))
            r = self._stream.drain()[0]
            if self.routes is None:
                return r.texts()
            out: List[Any] = [None] * len(lines)
            for i, x in self._routed_items(r):
                out[i] = x
            return out
        if times is not None:
            from .repeats import collapse_objects
            results = p.parse_lines(lines, **self._profile_kw())
            collapse_objects(results, times, self.window_us, self._carry)
            return results
        from .repeats import objects_key
        results = p.parse_lines(lines, collapse_repeats=True, **self._profile_kw())
        first = True
        for i, res in enumerate(results):
            k = objects_key(res)
            if k is None:
                continue
            if first and k == self._last_key:   # the batch's first decoding line repeats the previous batch's last
                results[i] = []
            first = False
            self._last_key = k
        return results

    def _parse_all(self, lines: List[Any], times: Optional[List[int]] = None) -> List[Any]:
        """publish='json_all' without the pipelined stream: one micro-batch through parse_lines_json_all -- with
        collapse_repeats through a json_all LineStream drained per batch, as _parse_collapsed does for 'json': its
        state carries the run of repeats from batch to batch, so both values of ``stream`` publish the same texts."""
        p = self.c.parser
        if not self.collapse:
            return p.parse_lines_json_all(lines, dispatch=self.rules, **self._profile_kw())
        if self._stream is None:
            kw = {} if times is None else {"repeat_window": self.window_us / 1e6}
            if self.rules is not None:
                kw["rules"] = self.rules
            self._stream = p.stream(chunk_lines=self.max_batch, output="json_all", lag=1, collapse_repeats=True, **kw,
                                    **self._profile_kw())
        self._stream.submit(lines, **({} if times is None else {"times": times}))
        return self._stream.drain()[0].texts_all()

    def _parse_routed(self, lines: List[Any]) -> List[Any]:
        kw = self._route_kw()
        return self.c.parser.parse_lines_routed(lines, kw.pop("routes"), **kw)

    def _parse_profiled(self, lines: List[Any]) -> List[Any]:
        p = self.c.parser
        return (p.parse_lines_json if self.publish == "json" else p.parse_lines)(lines, **self._profile_kw())

    async def run(self) -> None:
        c = self.c
        if self.use_stream:
            return await self._run_stream()
        while not c._stop_event.is_set():
            try:
                batch = await self._next_batch()
                lines = list(filter(None, batch))
                if lines:
                    parse = (self._parse_all if self.all else self._parse_collapsed if self.collapse else
                             self._parse_routed if self.routes is not None else
                             self._parse_profiled if self.profiles is not None else
                             c.parser.parse_lines_json if self.publish == "json" else c.parser.parse_lines)
                    times = self._times_of(batch)
                    results = await asyncio.to_thread(parse, lines, *([] if times is None else [times]))
                    self.batches += 1
                    for line, res in zip(lines, results):
                        if isinstance(res, Exception):  # parse_line raised for this line
                            self.logger.error("Parser error for line %r: %s", line, res)
                            res = None
                        if self.publish == "json":
                            if res is not None and c.mqtt_publisher:
                                await self._publish_json(res)
                        elif self.all:
                            if c.mqtt_publisher:
                                for text in res or []:   # the line's texts in order
                                    await self._publish_json(text)
                        else:
                            if res and c.message_callback:
                                await c.message_callback(res[0])
                            if c.mqtt_publisher and res:
                                await c.mqtt_publisher.publish(res[0])
                        if self._cmd_check():
                            await c._handle_as_command_response(line)
                    self.lines += len(lines)
                await asyncio.sleep(0)
            except asyncio.CancelledError:
                raise
            except Exception as e:  # noqa: BLE001  (controller.py:262-264)
                self.logger.error(f"Parser task error: {e}")
                break
