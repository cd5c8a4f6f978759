"""Stage 1 alone, for a kernel trace: query_vectors(packed=True) and pack_query_vectors at a few shapes,
both dtypes.  Run under rocprofv3 --kernel-trace --stats; the library comes from R_TUCKER_AMD_LIB."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import r_tucker_amd as rt
from r_tucker_amd import ops

dev = torch.device("cuda:0")
SHAPES = [   # (name, n_sub, n_rel, B, (a, b, c))
    ("c2", 40943, 22, 512, (10, 200, 200)),          # bench default: VALU tables, per-query contract
    ("c4b512", 14951, 2690, 512, (200, 200, 200)),   # FB15k B = 512: GEMM tables, planned, per-query contract with qinfo
    ("cfg4", 125000, 1000, 8192, (256, 512, 512)),   # BASELINE configs[4]: grouped contract
]
only = sys.argv[1] if len(sys.argv) > 1 else None
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
g = torch.Generator(device=dev).manual_seed(5)
for name, n_sub, n_rel, B, (a, b, c) in SHAPES:
    if only and only != name and only != "all":
        continue
    core = torch.randn((a, b, c), generator=g, device=dev) * (3.0 / (a * b * c) ** 0.5)
    R = torch.randn((n_rel, a), generator=g, device=dev)
    S = torch.randn((n_sub, b), generator=g, device=dev)
    h = torch.randint(0, n_sub, (B,), generator=g, device=dev)
    r = torch.randint(0, n_rel, (B,), generator=g, device=dev)
    for dt in (torch.float32, torch.bfloat16):
        cc, RR, SS = core.to(dt), R.to(dt), S.to(dt)
        for i in range(iters + 5):
            v, qp = ops.query_vectors(cc, RR, SS, h, r, packed=True)
            qp2 = ops.pack_query_vectors(v, dt)
        torch.cuda.synchronize()
        assert torch.equal(qp, qp2), (name, dt)     # the contract kernel's planes == pack_rows_kernel's on the same v
        print(name, dt, "ok", float(v.abs().max()), flush=True)
    del core, R, S
