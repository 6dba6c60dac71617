"""The timers the *_bench.py scripts share.  Each takes the torch module (the scripts import torch after parsing their arguments)
and a callable that enqueues the work, and returns microseconds per call, rounded to 0.1.  A script with a method of its own
(components_bench.py, simple_loops_bench.py, two_stage_bench.py, geometry_bench.py's wall) keeps it beside its use."""
import statistics
import time


def timed(torch, fn, iters, warmup):
    """Device events around `iters` calls after `warmup` calls: the median of three loops."""
    for _ in range(warmup):
        fn()
    loops = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        loops.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return round(statistics.median(loops), 1)


def timed_spread(torch, fn, iters, warmup):
    """(median, fastest, slowest) of three loops, microseconds per call."""
    for _ in range(warmup):
        fn()
    loops = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        loops.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return [round(statistics.median(loops), 1), round(min(loops), 1), round(max(loops), 1)]


def wall(torch, fn, iters, warmup):
    """Host clock around `iters` calls between two synchronisations: the median of three loops."""
    for _ in range(warmup):
        fn()
    loops = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        loops.append((time.perf_counter() - t0) * 1e6 / iters)
    return round(statistics.median(loops), 1)


def host_timed(torch, fn, iters):
    """Host clock around each of `iters` synchronised calls, no warm-up: the median call."""
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(out), 1)
