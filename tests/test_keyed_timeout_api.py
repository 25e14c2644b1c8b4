"""``stream.key_by(0).process(CountWithTimeout(timeout))`` (api/functions.py): the job on the
native timer operator against the host KeyedProcessOp (native off, a subclass, a key selector).
The events' timestamps are distinct, so no two deadlines tie and the outputs compare as lists."""
from __future__ import annotations

import pytest

from mxstream.api import functions as F
from mxstream.api.time import Time
from mxstream.api.tuples import Tuple2


def _env(native="auto", parallelism=4, device="cpu"):
    from mxstream.api.environment import StreamExecutionEnvironment
    from mxstream.api.time import TimeCharacteristic
    from mxstream.runtime.executor import ManualClock

    out = []
    env = StreamExecutionEnvironment(parallelism, clock=ManualClock(0)).set_output(out.append)
    env.config.native = native
    env.config.device = device
    env.set_stream_time_characteristic(TimeCharacteristic.EventTime)
    return env, out


def _samples():
    """Five hosts report every 10 s for 15 min; host3 is silent from 200 s to 500 s and host4
    stops at 300 s. Every timestamp is distinct."""
    events = []
    for i in range(450):
        h, t = i % 5, (i // 5) * 10_000 + (i % 5) * 7
        if (h == 3 and 200_000 <= t < 500_000) or (h == 4 and t >= 300_000):
            continue
        events.append((f"host{h}", float(i % 100), t))
    return events


SAMPLES = _samples()


class HostTimeout(F.CountWithTimeout):
    """A subclass keeps the host path: the planner lowers exactly CountWithTimeout."""


def first(v):
    """A key selector: the planner cannot see that it is field 0."""
    return v[0]


def _job(fn, native="auto", device="cpu", key=0):
    from mxstream.api.watermarks import BoundedOutOfOrdernessTimestampExtractor

    env, out = _env(native, device=device)
    env.from_timed_collection([(e[2] + 10, e) for e in SAMPLES]) \
        .assign_timestamps_and_watermarks(BoundedOutOfOrdernessTimestampExtractor(
            Time.milliseconds(0), extractor=lambda e: e[2])) \
        .map(lambda e: Tuple2(e[0], e[1])).key_by(key) \
        .process(fn).print()
    env.execute("silent-hosts")
    return out


def _expected() -> list:
    """(host, count, last) of every gap longer than 60 s and of the end of the input, replayed
    record by record; deadlines are distinct, so the output is in deadline order."""
    fired, count, last, armed = [], {}, {}, {}
    for host, _, t in SAMPLES:
        wm = t - 1  # the extractor's watermark after this element
        count[host] = count.get(host, 0) + 1
        last[host] = t
        armed[host] = t + 60_000
        for h in sorted(armed, key=armed.get):
            if armed[h] <= wm:
                fired.append((armed.pop(h), f"({h},{count[h]},{last[h]})"))
    fired.extend((d, f"({h},{count[h]},{last[h]})") for h, d in armed.items())
    return [text for _, text in sorted(fired)]


@pytest.fixture
def route(monkeypatch):
    from mxstream.runtime.native_ops import NativeTimeoutOp
    from mxstream.runtime.timeout_operator import KeyedTimeoutOperator

    seen = {"built": 0, "fallback": 0}
    init, to_fb = KeyedTimeoutOperator.__init__, NativeTimeoutOp._to_fallback

    def spy_init(self, *a, **kw):
        seen["built"] += 1
        init(self, *a, **kw)

    def spy_fb(self):
        seen["fallback"] += 1
        to_fb(self)

    monkeypatch.setattr(KeyedTimeoutOperator, "__init__", spy_init)
    monkeypatch.setattr(NativeTimeoutOp, "_to_fallback", spy_fb)
    return seen


def test_silent_host_job_native_on_cpu_equals_the_host_path(route):
    host = _job(HostTimeout(Time.seconds(60)))
    assert route == {"built": 0, "fallback": 0}
    rows = [ln[ln.index("("):] for ln in host]
    assert rows == _expected()
    # host3's gap, host4's stop, and the four hosts still reporting at the end of the input
    assert rows[0] == "(host3,20,190021)" and rows[1] == "(host4,30,290028)" and len(rows) == 6
    assert _job(F.CountWithTimeout(Time.seconds(60)), "off") == host
    assert route == {"built": 0, "fallback": 0}
    native = _job(F.CountWithTimeout(Time.seconds(60)))
    assert route == {"built": 1, "fallback": 0}
    assert native == host and len({ln[0] for ln in native}) > 1   # several subtasks print
    assert _job(F.CountWithTimeout(60_000)) == host


def test_selector_keys_keep_the_host_operator(route):
    got = _job(F.CountWithTimeout(Time.seconds(60)), key=first)
    assert route == {"built": 0, "fallback": 0}
    assert got == _job(HostTimeout(Time.seconds(60)))


def test_the_planner_marks_only_the_exact_class():
    from mxstream.api import planner

    metas = {}
    for name, fn, key in (("exact", F.CountWithTimeout(5), 0), ("sub", HostTimeout(5), 0),
                          ("selector", F.CountWithTimeout(5), first)):
        env, _ = _env()
        s = env.from_collection([("a", 1)]).key_by(key).process(fn)
        assert s.t.meta["kind"] == "keyed_process" and s.t.meta["fn"] is fn
        assert s.t.meta["key_pos"] == (0 if key == 0 else None)
        planner.plan(env, [s.t])
        metas[name] = bool(s.t.meta.get("native"))
    assert metas == {"exact": True, "sub": False, "selector": False}


def test_records_without_timestamps_raise_on_both_paths():
    from mxstream.runtime.executor import JobExecutionException

    for fn, native in ((F.CountWithTimeout(5), "auto"), (HostTimeout(5), "auto"),
                       (F.CountWithTimeout(5), "off")):
        env, _ = _env(native)
        env.from_collection([("a", 1)]).key_by(0).process(fn).print()
        with pytest.raises(JobExecutionException, match="ValueError: CountWithTimeout: a record "
                                                        "without an event timestamp") as e:
            env.execute("no-timestamps")
        assert isinstance(e.value.__cause__, ValueError)


def test_constructor_validation():
    assert F.CountWithTimeout(Time.seconds(2)).timeout == 2_000
    assert F.CountWithTimeout(7).native == ("count_timeout", 7)
    assert isinstance(F.CountWithTimeout(1), F.KeyedProcessFunction)
    for bad in (0, -1, True, False, 1.5, "60", None, Time.milliseconds(0), Time.seconds(-1)):
        with pytest.raises(ValueError, match="timeout"):
            F.CountWithTimeout(bad)


@pytest.mark.gpu
def test_gpu_silent_host_job_equals_the_host_path(gpu_device, route):
    host = _job(HostTimeout(Time.seconds(60)))
    got = _job(F.CountWithTimeout(Time.seconds(60)), device="cuda")
    assert route == {"built": 1, "fallback": 0}
    assert got == host and len(got) == 6
