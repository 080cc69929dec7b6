"""Microbench the fused BN / LN kernels at ResNet-50 / BERT-large shapes.

Prints per-kernel-group wall time (hipEvent) for bandwidth math; run
under `rocprofv3 --pmc FETCH_SIZE,SQ_LDS_BANK_CONFLICT,SQ_WAVES` for the
HBM-read bytes and LDS behavior (PMC runs must not add trace flags —
gpurun refuses the combination)."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from byteps_amd import ops as K  # noqa: E402

core = K.core()
ITERS = 50


def timed(label, fn, traffic_bytes):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / ITERS
    print("%-28s %8.1f us   %6.2f TB/s (of %.0f MB/iter)"
          % (label, ms * 1e3, traffic_bytes / ms / 1e9,
             traffic_bytes / 1e6), flush=True)


# the distinct BatchNorm shapes of ResNet-50 at batch 64 (N, C, H, W)
RESNET50_B64_BN = [
    (64, 64, 112, 112), (64, 256, 56, 56), (64, 128, 56, 56),
    (64, 512, 28, 28), (64, 64, 56, 56), (64, 256, 28, 28),
    (64, 1024, 14, 14), (64, 128, 28, 28), (64, 512, 14, 14),
    (64, 2048, 7, 7), (64, 256, 14, 14), (64, 512, 7, 7),
]


def bench_bn(N, C, H, W, apply=True):
    M = N * H * W
    x = torch.randn(N * H * W * C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    dy = torch.randn_like(x)
    dx = torch.empty_like(x)
    mask = torch.empty(M * C // 8, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(core.bn_stats_ws(M, C, 0), core.bn_stats_ws(M, C, 1)),
                     device="cuda")
    tickets = torch.zeros(2 * core.BN_TICKET_WORDS, dtype=torch.int32,
                          device="cuda")
    bwd_tickets = tickets.data_ptr() + 4 * core.BN_TICKET_WORDS
    mean = torch.empty(C, device="cuda")
    invstd = torch.empty(C, device="cuda")
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    g = torch.ones(C, device="cuda")
    b = torch.zeros(C, device="cuda")
    sums2 = torch.empty(2 * C, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    nbytes = M * C * 2
    tag = "bn[%d,%d,%d,%d]" % (N, C, H, W)

    timed(tag + " fwd_stats",
          lambda: core.bn_fwd_stats(x.data_ptr(), M, C, 1e-5, 0.1,
                                    mean.data_ptr(), invstd.data_ptr(),
                                    rm.data_ptr(), rv.data_ptr(), 1,
                                    ws.data_ptr(), tickets.data_ptr(), st),
          nbytes)
    core.bn_fwd_apply(x.data_ptr(), x.data_ptr(), y.data_ptr(), M, C,
                      mean.data_ptr(), invstd.data_ptr(), g.data_ptr(),
                      b.data_ptr(), 1, mask.data_ptr(), st)
    if apply:
        timed(tag + " fwd_apply(+res,relu)",
              lambda: core.bn_fwd_apply(x.data_ptr(), x.data_ptr(),
                                        y.data_ptr(), M, C, mean.data_ptr(),
                                        invstd.data_ptr(), g.data_ptr(),
                                        b.data_ptr(), 1, mask.data_ptr(), st),
              nbytes * 3)
    # bwd statistics read x, dy and the 1-byte-per-8-channels ReLU mask
    timed(tag + " bwd_stats(relu)",
          lambda: core.bn_bwd_stats(x.data_ptr(), dy.data_ptr(),
                                    mask.data_ptr(), M, C, mean.data_ptr(),
                                    invstd.data_ptr(), sums2.data_ptr(), 1,
                                    ws.data_ptr(), bwd_tickets, st),
          nbytes * 2 + M * C // 8)
    if apply:
        timed(tag + " bwd_apply(+dres,relu)",
              lambda: core.bn_bwd_apply(x.data_ptr(), dy.data_ptr(),
                                        mask.data_ptr(), dx.data_ptr(),
                                        y.data_ptr(), M, C, mean.data_ptr(),
                                        invstd.data_ptr(), g.data_ptr(),
                                        sums2.data_ptr(), 1, st),
              nbytes * 4)


def bench_ln(M, C):
    x = torch.randn(M * C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    dy = torch.randn_like(x)
    dx = torch.empty_like(x)
    g = torch.ones(C, device="cuda")
    b = torch.zeros(C, device="cuda")
    mean = torch.empty(M, device="cuda")
    invstd = torch.empty(M, device="cuda")
    nb = core.LN_RED_BLOCKS
    partial = torch.empty(nb * 2 * C, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    nbytes = M * C * 2
    tag = "ln[%d,%d]" % (M, C)
    timed(tag + " fwd",
          lambda: core.ln_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(),
                              y.data_ptr(), M, C, 1e-12, mean.data_ptr(),
                              invstd.data_ptr(), st),
          nbytes * 2)
    timed(tag + " bwd",
          lambda: core.ln_bwd(x.data_ptr(), dy.data_ptr(), g.data_ptr(),
                              mean.data_ptr(), invstd.data_ptr(),
                              dx.data_ptr(), M, C, partial.data_ptr(), st),
          nbytes * 3)


if __name__ == "__main__":
    # --stats: only the statistics kernels, at every ResNet-50 b64 shape
    stats_only = "--stats" in sys.argv
    for shape in RESNET50_B64_BN:
        bench_bn(*shape, apply=not stats_only)
    if not stats_only:
        bench_ln(64 * 128, 1024)       # BERT-large b64 s128
