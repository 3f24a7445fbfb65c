"""Where and when an entry point enqueues its work: the same call on a delayed side stream must give the bits of the plain call.

`run_on_side_stream(case)`:
  1. runs the entry on the default stream on the true inputs and keeps every output and every input buffer as it stands afterwards
     (`want`), then waits for the device;
  2. allocates live input buffers holding decoys (finite values that differ from the true ones; index-typed inputs need an explicit
     in-range decoy from the case: a wrong read gives wrong numbers, never a wild address) and output buffers filled with the
     byte 0x5A.  A case with a stateful object (trainer, sampler, bank) gets a second, fresh one; a case without runs the entry
     once on the decoys first, so that whatever the library or a Python wrapper keeps between calls (a cached workspace, a
     codec's activations) holds decoy-derived values and not the plain run's true ones;
  3. on a fresh `torch.cuda.Stream()` s enqueues one `torch.cuda._sleep` (one wave: every CU stays free, so a kernel launched
     anywhere else starts at once), an event, the copies of the true inputs into the live buffers, and the entry, called as users
     call it;
  4. notes whether the delay's event is still pending when the call returns;
  5. waits for s ALONE and compares bit for bit.  Nothing waits for the device between the call and the comparison: an internal
     stream that is not joined back into s stays visible.
A launch, memset or copy outside s, or a stage that is not ordered behind s, runs during the delay: it reads decoys, or its
output is overwritten later, and the bits differ.  A correct library passes whatever the timing; only the `pending` condition
depends on the delay's length.

The delay: DELAY_MS = 100.  `torch.cuda._sleep` counts device clock ticks: the ticks per millisecond are measured once per process
with two events (`sleep_cycles`; 2.4 million on the MI355X).  Measured there: the slowest case that does not synchronise is the
trainer's: 0.5 to 0.7 ms of host time for one forward_backward (micro, B = 2, T = 24), 2.1 ms at most for the case's whole
sequence (prepare, two forward_backward, optim, two EMA swaps, a re-pack); a model forward takes 0.2 ms, a single kernel entry
under 0.1 ms.  100 ms is 140 times the slowest call and about fifty times the slowest sequence.  Every synchronising entry
returned 100 to 112 ms after the delay was queued, i.e. when it ended.

What the harness cannot promise: a missing join of a library-owned stream BACK into s (s not waiting for that stream's last
work) shows only if that work is still running when s reaches its reader.  With the trainer's final join removed, the micro
trainer's last weight-gradient GEMMs finish before the caller's stream gets to the gradients and the cases pass; the missing
fork (the second stream not waiting for its operand) fails every trainer case.  DESIGN.md section 23 lists the mutations tried.

A case is a `Case`:
  inputs    {name: true tensor}, built on the default stream; each becomes a live buffer the entry reads (or updates in place)
  decoys    {name: tensor} for the inputs whose decoy cannot be derived (every integer or boolean input)
  outputs   {name: tensor} templates (shape, dtype) of caller-owned outputs; the entry sees sentinel-filled buffers
  state     optional callable (inputs, outputs) -> a fresh stateful object, called once per run before the delay starts, so the
            side run never sees what the plain run left behind
  call      call(state, inputs, outputs) -> None or {name: tensor} of further outputs (what a Python wrapper returns)
"""
import gc
import time

import torch

DELAY_MS = 100.0
SENTINEL = 0x5A

_cycles_per_ms = None


def sleep_cycles(ms):
    """`torch.cuda._sleep` ticks of `ms` milliseconds on this device, from one timed sleep per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)                      # first use: load the kernel
        torch.cuda.synchronize()
        probe = 20_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _cycles_per_ms = probe / max(a.elapsed_time(b), 1e-3)
        print(f"stream_check: torch.cuda._sleep runs {_cycles_per_ms:.0f} ticks per ms")
    return int(ms * _cycles_per_ms)


def _raw(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.uint8)


def bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(_raw(a), _raw(b))


def decoy_of(t):
    """A finite tensor of t's shape and dtype that differs from t nearly everywhere; floating point and complex only."""
    if t.is_complex():
        return torch.view_as_complex(decoy_of(torch.view_as_real(t)))
    if not t.dtype.is_floating_point:
        raise TypeError("an integer or boolean input needs an explicit in-range decoy")
    d = (t.flip(-1) if t.dim() else t).to(torch.float64) * 0.5 + 0.25
    return d.to(t.dtype).contiguous()


def sentinel_like(t):
    o = torch.empty_like(t, memory_format=torch.contiguous_format)
    if o.numel():
        (torch.view_as_real(o) if o.is_complex() else o).view(torch.uint8).fill_(SENTINEL)
    return o


class Case:
    def __init__(self, inputs, call, outputs=None, decoys=None, state=None):
        self.inputs, self.call, self.outputs = dict(inputs), call, dict(outputs or {})
        self.decoys, self.state = dict(decoys or {}), state

    def decoy(self, name):
        d = self.decoys[name] if name in self.decoys else decoy_of(self.inputs[name])
        assert d.shape == self.inputs[name].shape and d.dtype == self.inputs[name].dtype, name
        return d.contiguous().clone()


class Result:
    def __init__(self, mismatched, pending, host_ms):
        self.mismatched, self.pending, self.host_ms = mismatched, pending, host_ms

    def __repr__(self):
        return f"Result(mismatched={self.mismatched}, pending={self.pending}, host_ms={self.host_ms:.3f})"


def _gather(live, outs, ret):
    got = {"in:" + k: v for k, v in live.items()}
    got.update({"out:" + k: v for k, v in outs.items()})
    got.update({"ret:" + k: v for k, v in (ret or {}).items()})
    return got


def run_on_side_stream(case, delay_ms=DELAY_MS):
    assert torch.cuda.current_stream() == torch.cuda.default_stream(), "cases start on the default stream"
    # 1. the plain call
    live = {k: v.contiguous().clone() for k, v in case.inputs.items()}
    outs = {k: sentinel_like(v) for k, v in case.outputs.items()}
    st = case.state(live, outs) if case.state is not None else None
    ret = case.call(st, live, outs)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in _gather(live, outs, ret).items()}
    del live, outs, ret, st
    # 2. decoys in whatever is kept between calls, then live buffers with decoys, sentinel outputs, a second stateful object
    if case.state is None:
        case.call(None, {k: case.decoy(k) for k in case.inputs}, {k: sentinel_like(v) for k, v in case.outputs.items()})
        torch.cuda.synchronize()
    true = {k: v.contiguous() for k, v in case.inputs.items()}
    live = {k: case.decoy(k) for k in true}
    outs = {k: sentinel_like(v) for k, v in case.outputs.items()}
    st = case.state(live, outs) if case.state is not None else None
    cycles = sleep_cycles(delay_ms)
    # Objects of earlier cases that sit in reference cycles (a Trainer holds its own hook thunk) are destroyed by the cyclic
    # collector, whenever it next runs, and their destructors wait for the device (Trainer._release, the hipFree of a handle).
    # Collected here, and the collector held off while the side stream is being fed, that wait cannot land inside another
    # case's call and be taken for a synchronisation of the entry under test.
    gc.collect()
    torch.cuda.synchronize()
    # 3. delay, true inputs, the entry: all on s
    s = torch.cuda.Stream()
    end = torch.cuda.Event()
    collecting = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            end.record(s)
            for k in true:
                live[k].copy_(true[k], non_blocking=True)
            t0 = time.perf_counter()
            ret = case.call(st, live, outs)
            host_ms = (time.perf_counter() - t0) * 1e3
        # 4. did the call return before the delay ran out?
        pending = not end.query()
    finally:
        if collecting:
            gc.enable()
    # 5. s alone
    s.synchronize()
    got = _gather(live, outs, ret)
    bad = sorted(set(want) ^ set(got)) + [k for k in want if k in got and not bits_equal(want[k], got[k])]
    torch.cuda.synchronize()
    return Result(bad, pending, host_ms)


def check_case(case, name, synchronises=False):
    """The assertion of every case: equal bits, and the delay still pending at return unless the entry is listed as synchronising."""
    r = run_on_side_stream(case)
    print(f"{name}: host {r.host_ms:.3f} ms, delay pending at return: {r.pending}")
    assert not r.mismatched, f"{name}: the side-stream call differs from the plain call in {r.mismatched}"
    if not synchronises:
        assert r.pending, (f"{name}: inconclusive: the {DELAY_MS:.0f} ms delay had ended when the call returned after "
                           f"{r.host_ms:.1f} ms of host time (an undocumented synchronisation, or a delay that is too short)")
    return r
