"""python scripts/route_apply_time.py <missing rate> <accum>: ms per event-free 16-column apply at 500,000 x 100,000, one fresh process per
point.  The test build is loaded, so FPCA_I8_MODE (3: gathers, 0: two-matrix kernels) forces the route and FPCA_GATHER_BLOCKS the grid of
the gathers (0: the full grid; unset: the product's choice).  profiles/gather_resident_ab.txt, sections D."""
import os, sys, time
os.environ.setdefault("FPCA_LIB", "testhooks")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import flashpca_amd as fp

mr, accum = float(sys.argv[1]), sys.argv[2]
N, P, b = 500000, 100000, 16
with fp.Context.synthetic(N, P, n_pop=40, missing_rate=mr, accum=accum) as ctx:
    ctx.stats()
    rows = ctx.block_rows()
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    B = torch.zeros((rows, b), dtype=torch.float64, device="cuda")
    B[:N] = torch.rand((N, b), dtype=torch.float64, device="cuda", generator=g) - 0.5
    Y = torch.zeros((rows, b), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(10):
        ctx.apply_xxt_dev(B.data_ptr(), b, Y.data_ptr())
    ctx.synchronize()
    t0 = time.perf_counter()
    steps = 40
    for _ in range(steps):
        ctx.apply_xxt_dev(B.data_ptr(), b, Y.data_ptr())
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print("RESULT %.4f mode %d" % (ms, ctx.missing_mode(b)))
