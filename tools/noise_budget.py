"""Where is the float32 noise of the stage maps born?  (CPU experiment, literal oracle.)

Runs the literal restatement (oracle/lws_oracle.py) in float64 with ONE component at a time in float32 (inputs cast
down, result cast up) and reports each stage's max-abs distance to the all-float64 run.  The all-float32 line is the
reference algorithm's own noise floor.  Usage: python tools/noise_budget.py [--size 256x512] [--noise]

--per-op: instead, every per-op case of tests/float64_floor.py through the C restatement (oracle/lws_oracle.c, whose bits are the
HIP kernels' bits) against the literal oracle in float32 and float64, one line of ratios per gate and the worst per op: the
per-op table of DESIGN.md section 2.  --e2e: the end-to-end table beside it, from the committed tests/golden/ref_source_*.npz.
--split: the split-bf16 arithmetic restated on the CPU (oracle.lws_oracle.split_conv) on FF.SPLIT_CASES, six terms and each of
the three five-term forms: the emulation's lines of the same section (tests/test_float64_floor_cpu.py, part D, asserts them).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lwsnet_amd.synth import make_noise_pair, make_pair  # noqa: E402
from lwsnet_amd.weights import make_state_dict  # noqa: E402
from oracle import lws_oracle as O  # noqa: E402

COMPONENTS = ["features", "volume1", "conv3d_1", "regress1", "volume2", "conv3d_2", "regress2", "volume3", "conv3d_3",
              "regress3", "refine"]


def forward_mixed(left, right, sd, low=()):
    """float64 everywhere except the components named in `low` (float32)."""
    f64, f32 = torch.float64, torch.float32

    def dt(name):
        return f32 if name in low else f64

    left64 = torch.as_tensor(left, dtype=f64)
    right64 = torch.as_tensor(right, dtype=f64)
    H, W = left64.shape[2:]
    d = dt("features")
    fl = [f.to(f64) for f in O.feature_extraction(left64.to(d), sd, d)]
    fr = [f.to(f64) for f in O.feature_extraction(right64.to(d), sd, d)]
    pred = []
    mdl = [24, 5, 5]
    for s in range(3):
        h, w = fl[s].shape[2:]
        d = dt(f"volume{s + 1}")
        if s == 0:
            cost = O.build_volume_2d(fl[0].to(d), fr[0].to(d), mdl[0], d).to(f64)
        else:
            wflow = O._scale(O._interp(pred[s - 1].to(d), [h, w]) * float(h), H, d)
            cost = O.build_volume_2d3(fl[s].to(d), fr[s].to(d), mdl[s], wflow, d).to(f64)
        d = dt(f"conv3d_{s + 1}")
        c5 = cost.to(d).unsqueeze(1)
        cost = (O.post_3dconvs(c5, sd, s, d) + c5).squeeze(1).to(f64)
        d = dt(f"regress{s + 1}")
        p = F.softmax(-cost.to(d), dim=1)
        lowd = O.disparity_regression(p, 0 if s == 0 else -mdl[s] + 1, mdl[s], d)
        lowd = O._scale(lowd * float(H), lowd.shape[2], d)
        up = O._interp(lowd, [H, W])
        up = up if s == 0 else up + pred[s - 1].to(d)
        pred.append(up.to(f64))
    d = dt("refine")
    pred.append(O.refine(left64.to(d), pred[2].to(d), sd, d).to(f64))
    return pred


def per_op():
    """|C - fp64| over the gate's denominator (the literal float32 floor + tiny), whole tensor and border ring, per case."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import float64_floor as FF
    rows = []
    for family, cases in FF.CASES.items():
        for params in cases:
            c = FF.case(family, params)
            rows += [(family, label, r) for label, r in FF.check(c, FF.C_RUNNERS[family](c), show=lambda line: print(line, flush=True))]
    print(f"\n{'worst per op':19s} {'max':>5s} {'mean':>5s} {'ring max':>9s} {'ring mean':>10s}   (gates: {FF.MAX_FACTOR} / {FF.MEAN_FACTOR})")
    for family, r in FF.worst_per_family(rows).items():
        print(f"{family:19s} {r.max:5.2f} {r.mean:5.2f} {r.ring_max:9.2f} {r.ring_mean:10.2f}")


def split():
    """Ratios to the float32 floor of the six-term restatement and of the three five-term forms (ungated here), per split case."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import float64_floor as FF
    inf = float("inf")
    six, five = [], []
    for family, cases in FF.SPLIT_CASES.items():
        for mask, params in cases:
            c = FF.case(family, params)
            six += [(family, label, r) for label, r in FF.check(c, FF.split_emulation(c, mask), show=lambda line: print("six terms       " + line, flush=True))]
            for term in FF.ORDER2_TERMS:
                rows = FF.check(c, FF.split_emulation(c, mask, term), max_factor=inf, mean_factor=inf,
                                show=lambda line: print(f"without {term:8s}" + line, flush=True))
                if params in FF.SPLIT_TEETH[family]:
                    five += [(family, label, r) for label, r in rows]
    print(f"\n{'CPU emulation':32s} {'max':>5s} {'mean':>5s} {'ring max':>9s} {'ring mean':>10s}   (gates: {FF.MAX_FACTOR} / {FF.MEAN_FACTOR})")
    for family, r in FF.worst_per_family(six).items():
        print(f"{family + ', six terms, worst':32s} {r.max:5.2f} {r.mean:5.2f} {r.ring_max:9.2f} {r.ring_mean:10.2f}")
    for family in FF.SPLIT_TEETH:
        cols = [min(v for v in col if v is not None) for col in zip(*[r for f, _, r in five if f == family])]
        print(f"{family + ', five terms, smallest':32s} {cols[0]:5.2f} {cols[1]:5.2f} {cols[2]:9.2f} {cols[3]:10.2f}   (the cases of FF.SPLIT_TEETH)")


def e2e():
    """The distribution statistics of the C restatement's stage maps on the six reference-source fixtures."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import float64_floor as FF
    from oracle import c_oracle as C
    print(f"{'fixture':20s} stage  mean  median  |bias|  within 1e-3 px: build / reference float32")
    for name in FF.E2E_SMOOTH + FF.E2E_CHAOTIC:
        g, args, sd, align = FF.ref_source_case(name)
        with O.variant(align_mode=align):
            got = C.forward(g["left"], g["right"], sd, tuple(args.maxdisplist))
        for s in range(4):
            st = FF.assert_e2e_distribution(got[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} stage {s + 1}", None, None, None)
            print(f"{name:20s} {s + 1:5d} {st.mean_ratio:5.2f} {st.median_ratio:7.2f} {st.bias_ratio:7.2f}  {100 * st.within_1e3:6.2f} % / "
                  f"{100 * st.floor_within_1e3:6.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256x512")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--per-op", action="store_true", help="the per-op ratio table of the C restatement (tests/float64_floor.py)")
    ap.add_argument("--e2e", action="store_true", help="the end-to-end distribution table of the C restatement")
    ap.add_argument("--split", action="store_true", help="the split-bf16 emulation's ratio table (tests/float64_floor.py SPLIT_CASES)")
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    if a.per_op or a.e2e or a.split:
        if a.per_op:
            per_op()
        if a.split:
            split()
        if a.e2e:
            e2e()
        return
    H, W = (int(v) for v in a.size.split("x"))
    if a.noise:
        l, r = make_noise_pair(H, W, 0)
    else:
        l, r, _ = make_pair(H, W, 0)
    sd = make_state_dict(7)
    with torch.no_grad():
        ref = forward_mixed(l[None], r[None], sd, ())

        def report(name, low):
            p = forward_mixed(l[None], r[None], sd, low)
            e = [float((a_ - b_).abs().max()) for a_, b_ in zip(p, ref)]
            print(f"{name:12s} " + " ".join(f"{v:9.2e}" for v in e), flush=True)

        print(f"{'fp32 part':12s} " + " ".join(f"stage{s + 1:>4d}" for s in range(4)))
        report("ALL", tuple(COMPONENTS))
        for c in COMPONENTS:
            report(c, (c,))


if __name__ == "__main__":
    main()
