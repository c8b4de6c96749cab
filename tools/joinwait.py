"""Host-resolved joins of lws_forward at batch 1 (options host_joins / host_join_budget_us), one 256x512 pair:
  loop      400 forwards without a synchronise, three times per plan: host time per call, device-complete time per call, and per
            join (lws_join_stats) how it was resolved and how long the host polled (mean, longest) -- what the default budget
            comes from (profiles/NOTES.md, "Host-resolved joins")
  isolated  100 forwards with a synchronise before and after each: host time, latency, the same per-join figures
  latency   bench.py's latency pass (forward + synchronise, 50 samples), host_joins 0 and -1 alternating in ONE process, REPS
            blocks each: the p50 of such a block drifts by more than the effect between processes, alternation cancels it
Usage: python tools/joinwait.py [loop] [isolated] [latency[=REPS]]   (default: all three, 12 blocks)"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lwsnet_amd                                   # noqa: F401  (exports the runtime switches before HIP initialises)
import numpy as np
import torch
from lwsnet_amd import _lib
from lwsnet_amd.models import LWSNet
from lwsnet_amd.synth import make_batch
from lwsnet_amd.weights import default_args, make_state_dict

what = sys.argv[1:] or ["loop", "isolated", "latency"]
reps = next((int(w.split("=")[1]) for w in what if w.startswith("latency=")), 12)
dev = torch.device("cuda:0")
m = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
l, r = make_batch(1, 256, 512, 0)
l, r = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
lib = _lib.load()
default_budget = m.get_option("host_join_budget_us")


def stats():
    out = (ctypes.c_int64 * 12)()
    _lib.check(lib.lws_join_stats(m._h, out, 1), "lws_join_stats")
    return np.array(out[:]).reshape(3, 4)


def per_join(s):
    return "; ".join(f"join{j}: host {s[j, 0]} queued {s[j, 1]} mean {s[j, 2] / 1e3 / max(1, s[j, 0] + s[j, 1]):.1f} us "
                     f"max {s[j, 3] / 1e3:.1f} us" for j in range(3))


for _ in range(300):
    m(l, r)
torch.cuda.synchronize()
for hj, budget in ((0, default_budget), (1, 1000000), (-1, default_budget), (1, 100)):
    m.set_option("host_joins", hj)
    m.set_option("host_join_budget_us", budget)
    for _ in range(100):
        m(l, r)
    torch.cuda.synchronize()
    for rep in range(3 if "loop" in what else 0):
        stats()
        N = 400
        t0 = time.perf_counter()
        for _ in range(N):
            m(l, r)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"loop hj={hj} budget={budget}: host {1e6 * (t1 - t0) / N:.1f} us/call, device-complete {1e6 * (t2 - t0) / N:.1f} us/call "
              f"({N / (t2 - t0):.0f} pairs/s); {per_join(stats())}", flush=True)
    if "isolated" in what:
        stats()
        lat = []
        for _ in range(100):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m(l, r)
            th = time.perf_counter()
            torch.cuda.synchronize()
            lat.append((1e6 * (th - t0), 1e6 * (time.perf_counter() - t0)))
        lat = np.array(lat)
        print(f"isolated hj={hj} budget={budget}: host p50 {np.median(lat[:, 0]):.1f} us, latency p50 {np.median(lat[:, 1]):.1f} us "
              f"min {lat[:, 1].min():.1f}; {per_join(stats())}", flush=True)
m.set_option("host_join_budget_us", default_budget)
if any(w.startswith("latency") for w in what):
    p50 = {0: [], -1: []}
    for rep in range(reps):
        for hj in ((0, -1) if rep % 2 == 0 else (-1, 0)):
            m.set_option("host_joins", hj)
            m(l, r)
            torch.cuda.synchronize()
            lat = []
            for _ in range(50):
                t1 = time.perf_counter()
                m(l, r)
                torch.cuda.synchronize()
                lat.append(1e3 * (time.perf_counter() - t1))
            lat.sort()
            p50[hj].append(lat[25])
            print(f"latency block {rep} host_joins={hj}: p10 {lat[5]:.4f} p50 {lat[25]:.4f} p90 {lat[45]:.4f} ms", flush=True)
    a, b = np.array(p50[0]), np.array(p50[-1])
    print(f"latency p50 over {reps} alternating blocks: host_joins=0 median {np.median(a):.4f} ms ({a.min():.4f}..{a.max():.4f}), "
          f"automatic median {np.median(b):.4f} ms ({b.min():.4f}..{b.max():.4f}); automatic lower in {(b < a).sum()} of {reps} block pairs, "
          f"median of the pair differences {1e3 * np.median(b - a):+.1f} us")
