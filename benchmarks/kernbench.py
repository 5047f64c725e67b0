"""Microbenchmarks of the dfno_amd HIP kernels at flagship shapes.

Prints achieved GB/s (algorithmic bytes / wall) per kernel so regressions
against the ~6.3 TB/s HBM roofline are visible.  Dev tool, single GPU.
"""

import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dfno_amd import _ext  # noqa: E402

ext = _ext.get(required=True)


def bench(fn, *args, iters=20, warmup=5):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        fn(*args)
    torch.cuda.synchronize()
    return (time.time() - t0) / iters


def report(name, dt, bytes_):
    print(f"{name:44s} {dt*1e3:8.3f} ms   {bytes_/dt/1e12:6.2f} TB/s  ({bytes_/1e9:.2f} GB)")


def main():
    S = 64 * 64 * 64 * 30
    dev = "cuda"

    # channel mix fwd (block linear 20->20, no act)
    x = torch.randn(1, 20, S, device=dev)
    W = torch.randn(20, 20, device=dev)
    b0 = torch.empty(0, device=dev)
    dt = bench(lambda: ext.channel_mix_fwd(x, W, b0, False))
    report("channel_mix_fwd 20->20", dt, (20 + 20) * S * 4)

    # channel mix fwd 2->20 + gelu + z
    x2 = torch.randn(1, 2, S, device=dev)
    W2 = torch.randn(20, 2, device=dev)
    b2 = torch.randn(20, device=dev)
    dt = bench(lambda: ext.channel_mix_fwd(x2, W2, b2, True))
    report("channel_mix_fwd 2->20 gelu(+z)", dt, (2 + 40) * S * 4)

    # transposed (grad-x of 20->20)
    gz = torch.randn(1, 20, S, device=dev)
    dt = bench(lambda: ext.channel_mix_fwd_t(gz, W))
    report("channel_mix_fwd_t 20->20", dt, 40 * S * 4)

    # grad-W reduction 20x20
    dt = bench(lambda: ext.channel_mix_bwd_w(gz, x, False))
    report("channel_mix_bwd_w 20x20xS", dt, 40 * S * 4)

    # grad-W reduction 128x20 (proj head gW3)
    gz3 = torch.randn(1, 128, S, device=dev)
    dt = bench(lambda: ext.channel_mix_bwd_w(gz3, x, False))
    report("channel_mix_bwd_w 128x20xS", dt, (128 + 20) * S * 4)

    # proj head fwd 20->128->1
    W3 = torch.randn(128, 20, device=dev) / 20
    b3 = torch.randn(128, device=dev)
    W4 = torch.randn(1, 128, device=dev) / 128
    b4 = torch.randn(1, device=dev)
    dt = bench(lambda: ext.proj_head_fwd(x, W3, b3, W4, b4))
    report("proj_head_fwd 20->128->1", dt, 21 * S * 4)

    # proj head bwd
    gy = torch.randn(1, 1, S, device=dev)
    dt = bench(lambda: ext.proj_head_bwd(gy, x, W3, b3, W4))
    report("proj_head_bwd (gz3 write)", dt, (1 + 20 + 128) * S * 4)

    # fully-fused head backward (no gz3 in HBM; reads x+gy, writes gx)
    dt = bench(lambda: ext.proj_head_bwd_fused(gy, x, W3, b3, W4))
    report("proj_head_bwd_fused", dt, (20 + 1 + 20) * S * 4)
    # the two-output instantiation (O2T = 2)
    W42 = torch.randn(2, 128, device=dev) / 128
    gy2 = torch.randn(1, 2, S, device=dev)
    dt = bench(lambda: ext.proj_head_bwd_fused(gy2, x, W3, b3, W42))
    report("proj_head_bwd_fused, 2 outputs", dt, (20 + 2 + 20) * S * 4)
    del gy2

    # fused trunk mix backward (gz as an LDS tile; gz streamed = res grad)
    zmix = torch.randn(1, 20, S, device=dev)
    gymix = torch.randn(1, 20, S, device=dev)
    Wmix = torch.randn(20, 20, device=dev) / 20
    dt = bench(lambda: ext.channel_mix_bwd_fused(gymix, zmix, x, Wmix,
                                                 False, True))
    report("channel_mix_bwd_fused (+gz out)", dt, (3 * 20 + 2 * 20) * S * 4)
    # grad-x deferred to the rfft adjoint: no phase A, no gx store
    dt = bench(lambda: ext.channel_mix_bwd_fused(gymix, zmix, x, Wmix,
                                                 False, True, False))
    report("channel_mix_bwd_fused (gz out, no gx)", dt, (3 * 20 + 20) * S * 4)
    # the adjoint that takes it over: W^T gz + rfft_trunc_adj(G), T=30 m=8
    Gadj = torch.randn(1, 20, S // 30, 8, device=dev, dtype=torch.complex64)
    dt = bench(lambda: ext.rfft_adj_mix(gymix, Wmix, Gadj, 30))
    report("rfft_adj_mix", dt, (2 * 20 * S + 20 * (S // 30) * 16) * 4)

    # add gelu
    a = torch.randn(1, 20, S, device=dev)
    bb = torch.randn(1, 20, S, device=dev)
    dt = bench(lambda: ext.add_gelu_fwd(a, bb))
    report("add_gelu (y+z out)", dt, 80 * S * 4)

    # gelu bwd
    dt = bench(lambda: ext.gelu_bwd(a, bb))
    report("gelu_bwd", dt, 60 * S * 4)

    # spectral corners (two-phase block shapes, serial)
    F_ = (24, 24, 24, 8)
    xs = torch.randn(1, 20, *F_, device=dev, dtype=torch.complex64)
    ys = torch.zeros(1, 20, *F_, device=dev, dtype=torch.complex64)
    ws, starts = [], []
    m = (12, 12, 12, 8)
    for c in range(8):
        st = [(0 if (c >> d) & 1 == 0 else F_[d] - m[d]) for d in range(3)] + [0]
        ws.append(torch.randn(20, 20, *m, device=dev, dtype=torch.complex64) / 400)
        starts.append(st)
    wbytes = sum(w.numel() * 8 for w in ws)
    xbytes = xs.numel() * 8
    dt = bench(lambda: ext.spectral_corners_fwd(xs, ws, ys, starts))
    report("spectral_corners_fwd (8 corners)", dt, wbytes + 2 * xbytes)

    dt = bench(lambda: ext.spectral_corners_bwd_x(ys, ws, xs, starts))
    report("spectral_corners_bwd_x (8 corners)", dt, wbytes + 2 * xbytes)

    # grad-W + Adam of one block's corners: the two-kernel chain (gradient
    # written, then read back: 7 passes over the weights) against the fused
    # op (6 passes)
    gys = torch.randn(1, 20, *F_, device=dev, dtype=torch.complex64)
    gws = [torch.empty_like(w) for w in ws]
    ms = [torch.zeros_like(w) for w in ws]
    vs = [torch.zeros_like(w) for w in ws]
    flat = lambda ts: [torch.view_as_real(t).view(-1) for t in ts]
    pf, gf, mf, vf = flat(ws), flat(gws), flat(ms), flat(vs)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)

    def chain():
        ext.spectral_corners_bwd_w(xs, gys, gws, starts)
        ext.adam_step_batch_(pf, gf, mf, vf, *hyper, [1] * 8)

    dt = bench(chain)
    report("spectral_corners_bwd_w + adam_step_batch_", dt,
           7 * wbytes + 2 * xbytes)
    dt = bench(lambda: ext.spectral_gradw_adam_(xs, gys, ws, ms, vs, starts,
                                                *hyper, [1] * 8))
    report("spectral_gradw_adam_ (8 corners)", dt, 6 * wbytes + 2 * xbytes)

    # reference: raw copy bandwidth
    src = torch.randn(200_000_000 // 4, device=dev)
    dst = torch.empty_like(src)
    dt = bench(lambda: dst.copy_(src))
    report("torch copy_ 200MB (r+w)", dt, 2 * src.numel() * 4)


if __name__ == "__main__":
    if not {"--dft", "--lift", "--wide", "--wide-epilogue"} & set(sys.argv):
        main()


def dft_bench():
    """DFT kernels at flagship shapes."""
    # t-dim rfft: [1,20,64,64,64,30] -> m 8
    x = torch.randn(1, 20, 64, 64, 64, 30, device="cuda")
    dt = bench(lambda: ext.dft_rfft_trunc(x, 5, 8))
    report("dft_rfft_trunc t30->8", dt, (30 + 16) * 5242880 * 4)
    # z-dim c2c: [1,20,64,64,64,8] c64 -> 24
    xz = torch.randn(1, 20, 64, 64, 64, 8, device="cuda", dtype=torch.complex64)
    dt = bench(lambda: ext.dft_c2c(xz, 4, 64, 12, 12, True, 1.0))
    report("dft_c2c z64->24 analysis", dt, (64 + 24) * 8 * 20 * 64 * 64 * 8)
    dtS = bench(lambda: ext.dft_c2c(ext.dft_c2c(xz, 4, 64, 12, 12, True, 1.0), 4, 64, 12, 12, False, 1.0/64))
    report("dft_c2c z analysis+synthesis", dtS, 2 * (64 + 24) * 8 * 20 * 64 * 64 * 8)
    # y-dim c2c on truncated: [1,20,64,64,24,8]
    xy = torch.randn(1, 20, 64, 64, 24, 8, device="cuda", dtype=torch.complex64)
    dt = bench(lambda: ext.dft_c2c(xy, 3, 64, 12, 12, True, 1.0))
    report("dft_c2c y64->24 analysis", dt, (64 + 24) * 8 * 20 * 64 * 24 * 8)
    # irfft
    yt = torch.randn(1, 20, 64, 64, 64, 8, device="cuda", dtype=torch.complex64)
    dt = bench(lambda: ext.dft_pad_irfft(yt, 5, 30, 8))
    report("dft_pad_irfft 8->30", dt, (16 + 30) * 5242880 * 4)
    # torch reference: full rfft
    dt = bench(lambda: torch.fft.rfft(x, dim=5))
    report("torch rfft t30 (no trunc)", dt, (30 + 32) * 5242880 * 4)
    dt = bench(lambda: torch.fft.fft(xz, dim=4))
    report("torch fft z64 (no trunc)", dt, 2 * 64 * 8 * 20 * 64 * 64 * 8)


if "__main__" == __name__ and "--dft" in sys.argv:
    dft_bench()


def _alternate(fns, rounds=5, iters=50, all_rounds=False):
    """Time each fn in turn, `rounds` times over; median seconds per call
    (every round's time per fn with ``all_rounds``)."""
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(bench(fn, iters=iters, warmup=5))
    if all_rounds:
        return times
    return [sorted(t)[len(t) // 2] for t in times]


def lift_bench():
    """Fused lift head vs the composed linears, on identical inputs,
    alternating, in this one process.  Width 20: the Navier-Stokes shapes
    ([10,1,X,X,10] -> 40), per-rank X = 32 and single-GPU X = 64.  Width 64
    (the wide kernel rows): the flagship lift [1,2,64^3,1] -> 30 and the
    Navier-Stokes lift [10,1,64,64,10] -> 40, with every round listed: the
    fused route's slowest forward+backward round has to beat the composed
    route's fastest."""
    from dfno_amd.ops import lift_head
    from dfno_amd.ops.pointwise import linear_nd

    cases = [  # (B, C, spatial, Ti, To, W, iters)
        (10, 1, (32, 32), 10, 40, 20, 50),
        (10, 1, (64, 64), 10, 40, 20, 50),
        (1, 2, (64, 64, 64), 1, 30, 64, 10),
        (10, 1, (64, 64), 10, 40, 64, 20),
    ]
    for B, C, sp, Ti, To, W, iters in cases:
        S = 1
        for d in sp:
            S *= d
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(0)
            es = 4 if dtype == torch.float32 else 2
            x = torch.randn(B, C, *sp, Ti, device="cuda", dtype=dtype,
                            requires_grad=True)
            ws = [torch.randn(To, Ti, device="cuda", dtype=dtype) / Ti,
                  torch.randn(To, device="cuda", dtype=dtype),
                  torch.randn(W, C, device="cuda", dtype=dtype) / C,
                  torch.randn(W, device="cuda", dtype=dtype)]
            ws = [w.requires_grad_(True) for w in ws]
            gy = torch.randn(B, W, *sp, To, device="cuda", dtype=dtype)

            def fused():
                return lift_head(x, *ws)

            def composed():
                h = linear_nd(x, ws[0], ws[1], -1, "gelu")
                return linear_nd(h, ws[2], ws[3], 1, "gelu")

            def fb(f):
                return lambda: torch.autograd.grad(f(), [x] + ws, gy)

            with torch.no_grad():
                rf, rc = _alternate([fused, composed], iters=iters,
                                    all_rounds=True)
            rfb, rcb = _alternate([fb(fused), fb(composed)], iters=iters,
                                  all_rounds=True)
            tf, tc, tfb, tcb = (sorted(r)[len(r) // 2]
                                for r in (rf, rc, rfb, rcb))
            nin, nout = B * C * S * Ti, B * W * S * To
            tag = (f"W={W} S={'x'.join(str(d) for d in sp)} "
                   f"{str(dtype).split('.')[-1]}")
            report(f"lift fused    fwd      {tag}", tf, (nin + nout) * es)
            report(f"lift composed fwd      {tag}", tc, (nin + nout) * es)
            report(f"lift fused    fwd+bwd  {tag}", tfb, 2 * (nin + nout) * es + nin * es)
            report(f"lift composed fwd+bwd  {tag}", tcb, 2 * (nin + nout) * es + nin * es)
            if W > 24:
                ms = lambda r: [round(t * 1e3, 3) for t in r]  # noqa: E731
                print(f"  fwd rounds ms: fused {ms(rf)}  composed {ms(rc)}")
                print(f"  fwd+bwd rounds ms: fused {ms(rfb)}  composed "
                      f"{ms(rcb)}  slowest fused < fastest composed: "
                      f"{max(rfb) < min(rcb)}")
            del x, gy


def lift_model_bench():
    """fwd+bwd of the NS-shape model ([10,1,64,64,10] -> 40, width 20, 4
    blocks, one GPU) with the fused lift on and forced off, alternating."""
    import dfno_amd as dfno
    import dfno_amd.ops as ops

    gate, wide_gate = ops.lift_head_supported, ops.lift_head_wide_range
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1))
        model = dfno.DistributedFNONd(P_x, [10, 1, 64, 64, 10], 40, 20, (4, 4, 4),
                                      num_blocks=4, device=torch.device("cuda"),
                                      dtype=dtype)
        x = torch.rand(10, 1, 64, 64, 10, device="cuda", dtype=dtype)

        def step(on):
            def run():
                off = lambda *a: False  # noqa: E731
                ops.lift_head_supported = gate if on else off
                ops.lift_head_wide_range = wide_gate if on else off
                try:
                    model.zero_grad(set_to_none=True)
                    model(x).float().square().mean().backward()
                finally:
                    ops.lift_head_supported = gate
                    ops.lift_head_wide_range = wide_gate
            return run

        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            t_on, t_off = _alternate([step(True), step(False)], iters=20)
        name = str(dtype).split(".")[-1]
        print(f"NS model fwd+bwd {name}: fused lift {t_on*1e3:.3f} ms, "
              f"composed lift {t_off*1e3:.3f} ms")


if "__main__" == __name__ and "--lift" in sys.argv:
    lift_bench()
    lift_model_bench()


def wide_bench():
    """Wide channel mix (mix_wide.hip) at I = O = 64, B = 1, S = 64^3 * 30,
    fp32 and bf16.  The plain bias+GELU form runs against what served the
    shape before (the scalar LDS kernel behind channel_mix_fwd in fp32, the
    einsum composition in bf16), alternating, five rounds: the new kernel's
    slowest round has to beat the old route's fastest.  The residual+GELU
    form had no native route; it reports time and TB/s on x, res, y, z."""
    import torch.nn.functional as F

    S, C = 64 * 64 * 64 * 30, 64
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        es = 4 if dtype == torch.float32 else 2
        name = str(dtype).split(".")[-1]
        x = torch.randn(1, C, S, device="cuda", dtype=dtype)
        W = (torch.randn(C, C, device="cuda") / 8).to(dtype)
        b = torch.randn(C, device="cuda").to(dtype)
        e = torch.empty(0, device="cuda", dtype=dtype)

        def wide_plain():
            return ext.wide_channel_mix(x, W, b, e, True, False, True)

        if dtype == torch.float32:
            def old_plain():
                return ext.channel_mix_fwd(x, W, b, True)
        else:
            def old_plain():
                z = torch.einsum("oi,bis->bos", W, x) + b.view(1, -1, 1)
                return F.gelu(z), z

        tn, to = _alternate([wide_plain, old_plain], iters=10, all_rounds=True)
        nbytes = 3 * C * S * es                      # x, y, z
        report(f"wide mix bias+gelu {name} (median)", sorted(tn)[2], nbytes)
        report(f"old route bias+gelu {name} (median)", sorted(to)[2], nbytes)
        print(f"  wide rounds ms {[round(t * 1e3, 3) for t in tn]}  "
              f"old rounds ms {[round(t * 1e3, 3) for t in to]}  "
              f"slowest wide < fastest old: {max(tn) < min(to)}")
        del to

        res = torch.randn(1, C, S, device="cuda", dtype=dtype)
        (tr,) = _alternate([lambda: ext.wide_channel_mix(x, W, e, res, True,
                                                         False, True)], iters=10)
        report(f"wide mix res+gelu (x,res,y,z) {name}", tr, 4 * C * S * es)
        (tq,) = _alternate([lambda: ext.wide_channel_mix(x, W, e, res, True,
                                                         False, False)], iters=10)
        report(f"wide mix res+gelu, no z (x,res,y) {name}", tq, 3 * C * S * es)
        (tt,) = _alternate([lambda: ext.wide_channel_mix(x, W, e, e, False,
                                                         True, False)], iters=10)
        report(f"wide mix transposed (gz,gx) {name}", tt, 2 * C * S * es)
        del res


if "__main__" == __name__ and "--wide" in sys.argv:
    wide_bench()


def wide_epilogue_bench():
    """Fused irfft epilogue at I = O = 64 (fp32) against the pairs it
    replaces, alternating, five rounds, every round listed: a route wins when
    its slowest round beats the other's fastest.  Shapes: the flagship trunk
    (B = 1, S = 64^3 * 30, m = 8) and the width-64 Navier-Stokes trunk
    ([10, 64, 64, 64, 40], m = 4).
    Forward: irfft_linear_res_gelu_fwd (z stored) vs dft_pad_irfft +
    wide_channel_mix (res + GELU, z stored).
    Backward: rfft_adj_mix vs the transposed mix + dft_rfft_trunc_adj_acc,
    the transposed mix being the MFMA one the model takes at this width and,
    as a second partner, channel_mix_fwd_t."""
    C = 64
    e = torch.empty(0, device="cuda")
    ms = lambda r: [round(t * 1e3, 3) for t in r]  # noqa: E731
    for B, sp, N, m, iters in ((1, (64, 64, 64), 30, 8, 10),
                               (10, (64, 64), 40, 4, 20)):
        torch.manual_seed(0)
        L = 1
        for d in sp:
            L *= d
        S = L * N
        tag = f"B={B} S={'x'.join(str(d) for d in sp)}x{N} m={m}"
        act = B * C * S * 4
        spec = B * C * L * m * 8
        x = torch.randn(B, C, S, device="cuda")
        W = torch.randn(C, C, device="cuda") / 8
        Y = torch.randn(B, C, L, m, device="cuda", dtype=torch.complex64)

        def fused_fwd():
            return ext.irfft_linear_res_gelu_fwd(x, W, Y, N, True)

        def pair_fwd():
            r = ext.dft_pad_irfft(Y, 3, N, m).reshape(B, C, S)
            return ext.wide_channel_mix(x, W, e, r, True, False, True)

        tf, tp = _alternate([fused_fwd, pair_fwd], iters=iters, all_rounds=True)
        report(f"fused fwd (x,Y,y,z) {tag}", sorted(tf)[2], 3 * act + spec)
        report(f"irfft + wide mix fwd {tag}", sorted(tp)[2], 5 * act + spec)
        print(f"  fused rounds ms {ms(tf)}  pair rounds ms {ms(tp)}  "
              f"slowest fused < fastest pair: {max(tf) < min(tp)}")

        def fused_adj():
            return ext.rfft_adj_mix(x, W, Y, N)

        def pair_adj():
            g = ext.wide_channel_mix(x, W, e, e, False, True, False)[0]
            return ext.dft_rfft_trunc_adj_acc(Y, 3, N, g.reshape(B, C, L, N))

        def pair_adj_t():
            g = ext.channel_mix_fwd_t(x, W)
            return ext.dft_rfft_trunc_adj_acc(Y, 3, N, g.reshape(B, C, L, N))

        tf, tp, tt = _alternate([fused_adj, pair_adj, pair_adj_t], iters=iters,
                                all_rounds=True)
        report(f"fused adjoint (gz,G,gx) {tag}", sorted(tf)[2], 2 * act + spec)
        report(f"wide mix^T + rfft adj acc {tag}", sorted(tp)[2], 4 * act + spec)
        report(f"channel_mix_fwd_t + rfft adj acc {tag}", sorted(tt)[2],
               4 * act + spec)
        print(f"  fused rounds ms {ms(tf)}  wide pair rounds ms {ms(tp)}  "
              f"fwd_t pair rounds ms {ms(tt)}  slowest fused < fastest pair: "
              f"{max(tf) < min(min(tp), min(tt))}")
        del x, Y


if "__main__" == __name__ and "--wide-epilogue" in sys.argv:
    wide_epilogue_bench()
