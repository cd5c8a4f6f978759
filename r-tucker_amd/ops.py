"""Host side of the scoring path: tensor checks, workspace, stream, autograd.

``score_1vN`` is what ``score_fn(T)`` of both model flavours calls; it replaces the
five torch ops of ``src/model/asymmetric/R_TuckER.py:43-48`` with one call into the
C ABI (``rtk_score_1vN_f32`` / ``_bf16``).  Forward runs entirely in the hand-written
HIP kernels.  Backward (needed because the optimizer differentiates ``loss_fn(T)``,
``train.py:79-82``): the three B x N-sized steps -- logistic derivative, dO = dZ^T v,
dv = dZ O -- are HIP kernels (``rtk_sigmoid_grad_f32``, ``rtk_gemm_f32``,
``rtk_gemm_f32_splitk``); the small trilinear remainder (gradients of core, R, S from
dv) is device-side torch ops.  Nothing leaves the GPU.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import torch

from . import _lib

_workspaces = {}

# Logistic used by the fused score epilogue: "exact" = expf + IEEE divide (the formula
# torch's CPU kernel evaluates), "fast" = 1 / (1 + 2^(-z log2 e)) on v_exp_f32 + v_rcp_f32
# (1 ulp each; ~6x fewer VALU instructions).  Override with R_TUCKER_AMD_SIGMOID.
DEFAULT_SIGMOID = os.environ.get("R_TUCKER_AMD_SIGMOID", "fast")

# Row pitch of a freshly allocated score matrix, in elements.  Rows that start on a 128-byte
# boundary are written in full lines (and, in the bf16 kernel, with nontemporal stores): measured
# 5-20 % of the score kernel (tools/ubench/vmem_rate.hip).  With N not a
# multiple of the pitch unit the result is the (B, N) view of a (B, pitch) buffer, i.e. NOT
# contiguous; R_TUCKER_AMD_ROW_ALIGN=1 restores the dense layout.  The autograd path (training)
# always uses the dense layout.
ROW_ALIGN = max(1, int(os.environ.get("R_TUCKER_AMD_ROW_ALIGN", "32")))
# The two B x N sized backward products (dO = dZ^T v, dv = dZ O): "split_fp16" = three f16 MFMAs per k-step on
# hi/lo halves like the forward (normwise fp32-class accuracy), "f32" = the exact fp32 MFMA GEMM (5x slower).
BACKWARD_GEMM = os.environ.get("R_TUCKER_AMD_BWD_GEMM", "split_fp16")
# Training loss: "1" = BCE terms and the logit gradient's base written by the score kernel's epilogue (the B x N matrix
# is written once in the forward and read only by the backward GEMMs); "0" = scores, then two more passes over them.
FUSED_BCE = os.environ.get("R_TUCKER_AMD_FUSED_BCE", "1") == "1"


def _row_pitch(N, dtype):
    """Row pitch, in elements, of a fresh score buffer of N columns: rows start on 128-byte boundaries (ROW_ALIGN
    float32 elements; twice as many bf16 ones)."""
    unit = ROW_ALIGN * (4 // dtype.itemsize) if ROW_ALIGN > 1 else 1
    return -(-N // unit) * unit


def alloc_scores(B, N, device, lead=(), dtype=torch.float32):
    """(lead..., B, N) score buffer whose rows start on 128-byte boundaries (``_row_pitch``)."""
    pitch = _row_pitch(N, dtype)
    buf = torch.empty(tuple(lead) + (B, pitch), dtype=dtype, device=device)
    return buf[..., :N] if pitch != N else buf


def _require_gpu(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: r_tucker_amd scores on MI355X only (no CPU path; "
            "use the reference implementation or oracle/ for CPU runs)")


def _operand(name, t, dtype):
    _require_gpu(name, t)
    if t.dtype != dtype:
        raise RuntimeError(f"{name} is {t.dtype} but the core is {dtype}: all operands must share one dtype "
                           "(float32, or bfloat16 for the bf16 path)")
    return t.contiguous()


def _idx(name, t, device):
    if isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device == device and t.dim() == 1 and t.is_contiguous():
        return t
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise IndexError(f"{name} must be an integer tensor, got {t.dtype}")  # torch: "tensors used as indices must be long..."
    return t.to(device=device, dtype=torch.int64).contiguous().view(-1)


def _dtype_code(bf16):
    return _lib.RTK_BF16 if bf16 else _lib.RTK_F32


def _entry(name, bf16):
    """The bf16 or the f32 form of a C-ABI entry point (``name_bf16`` / ``name_f32``)."""
    return getattr(_lib.load(), name + ("_bf16" if bf16 else "_f32"))


def _ld(t):
    """The row pitch of a (rows, cols) matrix as the C ABI takes it: its row stride, or cols for at most one row."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _wants_grad(*tensors):
    """Whether autograd is recording and one of ``tensors`` asks for a gradient."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _f32(*operands):
    """The fp32 operands a backward computes with: bf16 operands (they share one dtype) upcast, fp32 ones as they are."""
    return operands if operands[0].dtype == torch.float32 else tuple(t.float() for t in operands)


def _grads_like(grads, dtype):
    """Gradients computed in fp32, returned in the operands' ``dtype`` (None stays None)."""
    return tuple(grads) if dtype == torch.float32 else tuple(None if g is None else g.to(dtype) for g in grads)


def _zero_batch_grads(ctx):
    """The backward of an empty batch (core, R, S, O saved first): zero gradients of each operand's shape and dtype for
    the operands that want one, nothing launched."""
    needs = ctx.needs_input_grad
    return tuple(torch.zeros_like(t) if n else None for t, n in zip(ctx.saved_tensors, needs[:4])) + (None,) * (len(needs) - 4)


def _spend(ctx, who, stored):
    """One backward per forward of a stored-matrix loss: its backward overwrites the saved matrix."""
    if getattr(ctx, "spent", False):
        raise RuntimeError(f"{who}: backward called twice (the saved {stored} are overwritten by the first pass)")
    ctx.spent = True


class _Operands:
    """The checked operands of one call: core (a, b, c) and, when given, R, S, O and the index vectors h, r of B queries;
    contiguous, on one GPU, in one dtype, with matching widths (the C ABI takes a, b, c from the core alone)."""
    __slots__ = ("core", "R", "S", "O", "h", "r", "a", "b", "c", "B", "dev", "bf16", "dcode")

    def __init__(self, core, R, S=None, O=None, subject_idx=None, relation_idx=None):
        _require_gpu("core", core)
        dt = core.dtype
        if dt not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"core must be float32 or bfloat16, got {dt}")
        self.bf16 = dt == torch.bfloat16
        self.dcode = _dtype_code(self.bf16)
        self.core = core = core.contiguous()
        self.R = R = None if R is None else _operand("R", R, dt)
        self.S = S = None if S is None else _operand("S", S, dt)
        self.O = O = None if O is None else _operand("O", O, dt)
        self.dev = dev = core.device
        for n, t in (("R", R), ("S", S), ("O", O)):
            if t is not None and t.device != dev:
                raise RuntimeError(f"{n} is on {t.device}, core on {dev}")
        if core.dim() != 3 or any(t is not None and t.dim() != 2 for t in (R, S, O)):
            raise RuntimeError("expected core (a,b,c), R (nR,a), S (N,b), O (N,c)")
        self.a, self.b, self.c = a, b, c = core.shape
        if (R is not None and R.shape[1] != a) or (S is not None and S.shape[1] != b) or (O is not None and O.shape[1] != c):
            raise RuntimeError("factor widths " + ", ".join(f"{n} {t.shape[1]}" for n, t in (("R", R), ("S", S), ("O", O))
                                                            if t is not None) + f" do not match core {tuple(core.shape)}")
        self.h = self.r = None
        self.B = 0
        if subject_idx is not None:
            self.h, self.r = _idx("subject_idx", subject_idx, dev), _idx("relation_idx", relation_idx, dev)
            if self.h.numel() != self.r.numel():
                raise RuntimeError(f"subject_idx has {self.h.numel()} entries, relation_idx {self.r.numel()}")
            self.B = self.h.numel()
        if b != c:
            # asymmetric/R_TuckER.py:46: .view(-1, b) of a (B,1,c) tensor
            raise RuntimeError(f"shape '[-1, {b}]' is invalid for input of size {self.B * c}" if self.h is not None
                               else f"subject rank {b} must equal object rank {c} (asymmetric/R_TuckER.py:46)")

    def workspace(self, sp, tables=None):
        """The workspace of a stage 1 on stream ``sp``, from the relation ``tables`` when given, else from the core."""
        n_rel = self.R.shape[0]
        need = (_size("rtk_from_tables_workspace_bytes", self.B, n_rel) if tables is not None
                else _size("rtk_workspace_bytes", self.dcode, self.B, n_rel, self.a, self.b, self.c))
        return _workspace(self.dev, sp, need)

    def check_tables(self, tables):
        n_rel = self.R.shape[0]
        if (not isinstance(tables, torch.Tensor) or tables.dtype != torch.float32 or tables.device != self.dev
                or tuple(tables.shape) != (n_rel, self.b, self.c) or not tables.is_contiguous()):
            raise RuntimeError(f"tables must be a contiguous float32 ({n_rel}, {self.b}, {self.c}) tensor on {self.dev} "
                               "(ops.relation_tables)")


_sizes = {}      # memoised size queries of the C ABI (one ctypes call each otherwise, per scoring call)
_packed = {}     # (device index, stream) -> packed-query-plane buffer of the calls that do not hand the planes out


def _size(fn_name, *args):
    key = (fn_name,) + args
    v = _sizes.get(key)
    if v is None:
        v = _sizes[key] = getattr(_lib.load(), fn_name)(*args)
    return v


def _packed_buffer(device, stream_ptr, nbytes):
    """Packed query planes of a call that does not hand them out: written by stage 1 and read by the score kernel
    of the same call on the same stream, so one buffer per (device, stream) serves every call (no allocation)."""
    key = (device.index, stream_ptr)
    b = _packed.get(key)
    if b is None or b.numel() < nbytes:
        b = _packed[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    return b


def _workspace(device, stream_ptr, nbytes):
    """The caller-owned scratch of the C ABI, one per (device, stream).  Its 256-byte header holds the
    sticky device error word (include/rtucker_hip.h); when the buffer has to grow the header is carried
    over, so an out-of-range id seen before the regrow is still reported.  Called with the owning
    stream current, so the header copy is ordered behind the kernels that may have set the word."""
    key = (device.index, stream_ptr)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        new = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        if ws is None:
            new[:256].zero_()
        else:
            new[:256].copy_(ws[:256])
        _workspaces[key] = ws = new
    return ws


# What happens when a kernel meets an out-of-range subject / relation id (the kernels clamp it and raise
# a sticky flag; the reference raises IndexError, SURVEY.md section 8b "Errors"):
#   "strict"   (default) every scoring call reads the flag back before returning -> IndexError like the
#              reference, at the price of one stream synchronisation per call;
#   "deferred" nothing per call; ``check_device_errors()`` raises at the caller's own sync point
#              (``evaluate()`` and the training driver do that once per loop);
#   "off"      never checked (graph capture, benchmarks).
# Calls made while the stream is being captured into a HIP graph are never synchronised.
INDEX_CHECK = os.environ.get("R_TUCKER_AMD_INDEX_CHECK", "strict")


class index_check:
    """Context manager / setter for the out-of-range-id policy: ``with index_check("deferred"): ...``."""

    def __init__(self, mode):
        if mode not in ("strict", "deferred", "off"):
            raise ValueError(f"index check mode must be strict | deferred | off, got {mode!r}")
        self.mode = mode

    def __enter__(self):
        global INDEX_CHECK
        self.prev, INDEX_CHECK = INDEX_CHECK, self.mode
        return self

    def __exit__(self, *exc):
        global INDEX_CHECK
        INDEX_CHECK = self.prev
        return False


def _check_now(ws, sp):
    """Read (and clear) the error word of one workspace on its own stream; raise like torch's indexing."""
    flag = C.c_uint32(0)
    _lib.check(_lib.load().rtk_read_error_flag(ws.data_ptr(), sp, C.byref(flag)), "rtk_read_error_flag")
    if flag.value & 1:
        raise IndexError("index out of range in self (subject_idx / relation_idx)")
    if flag.value & 2:
        raise IndexError("index out of range in self (candidate id out of range)")
    if flag.value & 4:
        raise IndexError("index out of range in self (object_idx out of range)")
    if flag.value & 8:
        raise RuntimeError("bce_loss_1vN(matrix_free=True): the batch's queries list more known objects than max_pos "
                           "(pass a larger max_pos)")


def _strict_check(ws, sp):
    if INDEX_CHECK == "strict" and not torch.cuda.is_current_stream_capturing():
        _check_now(ws, sp)


def _stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


# Largest object rank c of the score kernels on packed query planes (rtk_score_packed_*; the library's own rule is
# rtk_split_ksteps_supported, csrc/rtk_score_select.h).  Above it, and for exact=True, stage 2 is the exact-fp32
# rtk_score_f32 on the unpacked query vectors, which exists for fp32 operands only.
_PACKED_MAX_C = 512


def _packed_stage2(c, exact):
    """Whether the score kernel can run on packed query planes."""
    return not exact and c <= _PACKED_MAX_C


def _score_flags(sigmoid, sigmoid_mode, out_dtype, bf16):
    """The score kernel's flags (logistic, its mode, bf16 output) for scores in ``out_dtype``."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    mode = sigmoid_mode or DEFAULT_SIGMOID
    if mode not in ("fast", "exact"):
        raise ValueError(f"sigmoid mode must be 'fast' or 'exact', got {mode!r}")
    flags = (_lib.RTK_SCORE_SIGMOID | (_lib.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)) if sigmoid else 0
    if out_dtype == torch.bfloat16:
        if not bf16 or not sigmoid or mode != "fast":
            raise RuntimeError("bfloat16 scores: bf16 operands, sigmoid=True and the fast logistic (sigmoid_mode='fast')")
        flags |= _lib.RTK_SCORE_OUT_BF16
    return flags


def _stage1(op, sp, tables, v, qp):
    """Stage 1: the query vectors into ``v`` (B, c) fp32 and / or their packed planes into ``qp`` (either may be None),
    from the relation ``tables`` when given, else from the core.  Returns the workspace (the error word's holder)."""
    n_rel = op.R.shape[0]
    vp, qpp = (None if v is None else v.data_ptr()), (None if qp is None else qp.data_ptr())
    ws = op.workspace(sp, tables)
    if tables is not None:
        op.check_tables(tables)
        _lib.check(_entry("rtk_query_vectors_from_tables", op.bf16)(
            tables.data_ptr(), n_rel, op.b, op.c, op.S.data_ptr(), op.S.shape[0], op.r.data_ptr(), op.h.data_ptr(), op.B,
            vp, qpp, ws.data_ptr(), ws.numel(), sp), "rtk_query_vectors_from_tables")
    else:
        _lib.check(_entry("rtk_query_vectors", op.bf16)(
            op.core.data_ptr(), op.a, op.b, op.c, op.R.data_ptr(), n_rel, op.S.data_ptr(), op.S.shape[0],
            op.r.data_ptr(), op.h.data_ptr(), op.B, vp, qpp, ws.data_ptr(), ws.numel(), sp), "rtk_query_vectors")
    return ws


def _stage2(bf16, sp, v, qp, O, out, flags):
    """Stage 2: the scores ``out`` (B, N) against ``O`` from the packed planes ``qp``, or, when there are none, from
    ``v`` (``rtk_score_f32``, which takes the sigmoid flag alone)."""
    B, N = out.shape
    ld = _ld(out)
    if qp is not None:
        _lib.check(_entry("rtk_score_packed", bf16)(qp.data_ptr(), B, O.shape[1], O.data_ptr(), N, out.data_ptr(), ld,
                                                    flags, sp), "rtk_score_packed")
    else:
        _lib.check(_lib.load().rtk_score_f32(v.data_ptr(), B, O.shape[1], O.data_ptr(), N, out.data_ptr(), ld,
                                             flags & _lib.RTK_SCORE_SIGMOID, sp), "rtk_score_f32")


def relation_tables(core, R):
    """``tables[u] = G x_0 R[u]`` for ALL relations -> ``(n_rel, b, c)`` fp32: the part of stage 1 that only
    depends on the parameters (einsum of asymmetric/R_TuckER.py:45 applied to every relation row).  Pass the
    result as ``tables=`` to ``score_1vN`` / ``query_vectors`` while the parameters stay unchanged."""
    op = _Operands(core, R)
    a, b, c, n_rel, dev = op.a, op.b, op.c, op.R.shape[0], op.dev
    tables = torch.empty((n_rel, b, c), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(_lib.load().rtk_relation_tables_workspace_bytes(op.dcode, n_rel, a, b, c), dtype=torch.uint8,
                              device=dev)
        _lib.check(_entry("rtk_relation_tables", op.bf16)(op.core.data_ptr(), a, b, c, op.R.data_ptr(), n_rel,
                                                          tables.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                          _stream_ptr(dev)), "rtk_relation_tables")
    return tables


def _forward(core, R, S, O, subject_idx, relation_idx, sigmoid, exact, want_v, sigmoid_mode=None, out=None,
             out_dtype=torch.float32, padded=None, tables=None):
    op = _Operands(core, R, S, O, subject_idx, relation_idx)
    flags = _score_flags(sigmoid, sigmoid_mode, out_dtype, op.bf16)
    if out_dtype == torch.bfloat16 and (want_v or exact):
        raise RuntimeError("bfloat16 scores: bf16 operands, sigmoid=True, no autograd (the reference's bf16 eval path)")
    B, N, dev = op.B, op.O.shape[0], op.dev
    if out is None:
        # dense when the scores are handed to autograd's caller, 128-byte aligned rows otherwise
        dense = want_v if padded is None else not padded
        out = torch.empty((B, N), dtype=torch.float32, device=dev) if dense else alloc_scores(B, N, dev, dtype=out_dtype)
    elif (tuple(out.shape) != (B, N) or out.dtype != out_dtype or out.device != dev or out.stride(1) != 1
          or out.stride(0) < N):
        raise RuntimeError(f"out must be a {out_dtype} ({B}, {N}) tensor on {dev} with unit column stride")
    if B == 0:
        return out, None, op
    packed = _packed_stage2(op.c, exact)
    if op.bf16 and not packed:
        raise RuntimeError(f"bf16 operands: only the bf16 MFMA score kernel exists (c <= {_PACKED_MAX_C}, exact=False)")
    v = None
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        if tables is None and not want_v:
            ws = op.workspace(sp)
            _lib.check(_entry("rtk_score_1vN", op.bf16)(
                op.core.data_ptr(), op.a, op.b, op.c, op.R.data_ptr(), op.R.shape[0], op.S.data_ptr(), op.S.shape[0],
                op.O.data_ptr(), N, op.r.data_ptr(), op.h.data_ptr(), B, out.data_ptr(), _ld(out),
                flags | (_lib.RTK_SCORE_EXACT_F32 if exact else 0), ws.data_ptr(), ws.numel(), sp), "rtk_score_1vN")
        else:
            # two calls: the fp32 query vectors are kept for backward, or stage 1 reads the relation tables
            v = torch.empty((B, op.c), dtype=torch.float32, device=dev) if want_v or not packed else None
            qp = _packed_buffer(dev, sp, _size("rtk_packed_query_bytes", op.dcode, B, op.c)) if packed else None
            ws = _stage1(op, sp, tables, v, qp)
            _stage2(op.bf16, sp, v, qp, op.O, out, flags)
        _strict_check(ws, sp)
    return out, v, op


class _Score1vN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, core, R, S, O, subject_idx, relation_idx, sigmoid, exact, sigmoid_mode):
        out, v, op = _forward(core, R, S, O, subject_idx, relation_idx, sigmoid, exact, want_v=True, sigmoid_mode=sigmoid_mode)
        ctx.save_for_backward(op.core, op.R, op.S, op.O, op.h, op.r, v, out)
        ctx.sigmoid = sigmoid
        return out

    @staticmethod
    def backward(ctx, grad_out):
        core, R, S, O, h, r, v, out = ctx.saved_tensors
        B, N = out.shape
        if B == 0:
            return _zero_batch_grads(ctx)
        lib = _lib.load()
        dev = out.device
        grad_out = grad_out.contiguous().float()
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            if ctx.sigmoid and B > 65535:   # (the row-pitch kernel's grid limit) dense dZ
                dZ = torch.empty_like(out)
                _lib.check(lib.rtk_sigmoid_grad_f32(grad_out.data_ptr(), out.data_ptr(), dZ.data_ptr(), out.numel(), sp),
                           "rtk_sigmoid_grad_f32")
            elif ctx.sigmoid:    # dZ = dP * P * (1 - P)   (HIP), written on 128-byte aligned rows for the GEMMs
                dZ = alloc_scores(B, N, dev)
                _lib.check(lib.rtk_sigmoid_grad_rows_f32(grad_out.data_ptr(), N, out.data_ptr(), _ld(out), dZ.data_ptr(), _ld(dZ),
                                                         B, N, sp), "rtk_sigmoid_grad_rows_f32")
            else:
                dZ = grad_out
        return _grads_from_dZ(core, R, S, O, h, r, v, dZ, ctx.needs_input_grad) + (None,) * 5


def _splits_for(M, N, K):
    """Split-K factor of the dv product: enough 128x128 tiles x chunks to fill 256 CUs twice, chunks >= 512 deep."""
    tiles = -(-M // 128) * -(-N // 128)
    return int(max(1, min(64, 512 // max(tiles, 1), K // 512)))


def _grads_from_dZ(core, R, S, O, h, r, v, dZ, needs, dz_bound=None, scale=None):
    """(g_core, g_R, g_S, g_O) from dZ = d loss / d logits (B, N) fp32, the operands as the forward saved them (bf16
    ones: computed in fp32, returned in bf16) and the saved fp32 query vectors, all in HIP kernels with a fixed
    summation order (bit-identical from run to run): dO = dZ^T v and dv = dZ O (split-K slabs added in chunk order) on the split-fp16 MFMA path of the forward
    (``BACKWARD_GEMM = "f32"`` / ``R_TUCKER_AMD_BWD_GEMM=f32``: the exact fp32 MFMA GEMM), then the stage-1
    backward ``rtk_query_vectors_bwd_f32`` (two more GEMMs and a deterministic row scatter; above 1 GiB of workspace its
    stream form, ``stage1_backward_route``).  ``dz_bound``: a
    one-element device tensor >= max|dZ| when the caller knows one (the BCE gradient does); otherwise one
    max-reduction over dZ finds it.  ``scale``: a one-element device tensor s -- the gradients of ``s * dZ`` are
    returned without a pass over dZ: everything is linear in dZ, so s multiplies the small operands
    (``v`` for dO, ``dv`` before the stage-1 backward)."""
    lib = _lib.load()
    dev = dZ.device
    B, N = dZ.shape
    ldz = _ld(dZ)                           # dZ may be the (B, N) view of a padded buffer (bce_loss_1vN)
    a, b, c = core.shape
    pdt = core.dtype
    # (core, R and S go to the stage-1 backward as they are: it makes its fp32 copies only on the route that needs them)
    Of = (O if pdt == torch.float32 else O.float()).contiguous()
    gO = gcore = gR = gS = None
    sf16 = BACKWARD_GEMM != "f32"
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        if sf16:
            bounds = torch.empty(3, dtype=torch.float32, device=dev)      # max|dZ|, max|v|, max|O|

            def absmax(x, ld, slot):
                _lib.check(lib.rtk_absmax_f32(x.data_ptr(), x.shape[0], x.shape[1], ld, bounds[slot:].data_ptr(), sp),
                           "rtk_absmax_f32")
                return bounds[slot:slot + 1]
            if dz_bound is None:
                dz_bound = absmax(dZ, ldz, 0)
            dz_bound = dz_bound.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        v_o = v if scale is None else v * scale.to(device=dev, dtype=torch.float32).reshape(1)      # (B, c): dO's small operand
        if sf16:
            v_bound = absmax(v_o, c, 1)
        if needs[3]:
            # gO[j, k] = sum_d dZ[d, j] * v[d, k]   -- fp32 MFMA GEMM, both operands M-major
            gO = torch.empty((N, c), dtype=torch.float32, device=dev)
            if sf16:
                _lib.check(lib.rtk_gemm_sf16_splitk(dZ.data_ptr(), 0, ldz, dz_bound.data_ptr(), v_o.data_ptr(), 0, c,
                                                    v_bound.data_ptr(), gO.data_ptr(), c, N, c, B, 1, None, 0, sp),
                           "rtk_gemm_sf16_splitk (dO)")
            else:
                _lib.check(lib.rtk_gemm_f32(dZ.data_ptr(), 0, ldz, v_o.data_ptr(), 0, c, gO.data_ptr(), c, N, c, B, 0, sp),
                           "rtk_gemm_f32 (dO)")
        if needs[0] or needs[1] or needs[2]:
            # dv[d, k] = sum_j dZ[d, j] * O[j, k]   -- K = N entities: split-K, slabs reduced in chunk order
            dv = torch.empty((B, c), dtype=torch.float32, device=dev)
            splits = _splits_for(B, c, N)
            skw = torch.empty(max(256, lib.rtk_gemm_f32_splitk_workspace_bytes(B, c, splits)), dtype=torch.uint8, device=dev)
            if sf16:
                o_bound = absmax(Of, c, 2)
                _lib.check(lib.rtk_gemm_sf16_splitk(dZ.data_ptr(), 1, ldz, dz_bound.data_ptr(), Of.data_ptr(), 0, c,
                                                    o_bound.data_ptr(), dv.data_ptr(), c, B, c, N, splits, skw.data_ptr(),
                                                    skw.numel(), sp), "rtk_gemm_sf16_splitk (dv)")
            else:
                _lib.check(lib.rtk_gemm_f32_splitk(dZ.data_ptr(), 1, ldz, Of.data_ptr(), 0, c, dv.data_ptr(), c, B, c, N,
                                                   splits, skw.data_ptr(), skw.numel(), sp), "rtk_gemm_f32_splitk (dv)")
            if scale is not None:
                dv = dv * scale.to(device=dev, dtype=torch.float32).reshape(1)
            gcore, gR, gS = _stage1_backward(core, R, S, h, r, dv, needs)
    # symmetric model: S and O are the same tensor passed twice; autograd sums gS + gO
    return _grads_like((gcore, gR, gS, gO), pdt)


class _GramTN(torch.autograd.Function):
    """``A^T B`` for tall-skinny fp32 GPU operands ``A (n, p)``, ``B (n, q)``, ``n >> p, q`` -- the Gram-type
    products of the Riemannian layer (factor Gram matrices in ``T.norm()``, ``U^T M`` in the tangent-space
    projection; n = 40 943, p = q = 400 at the WN18RR training shape).  rocBLAS runs this shape on
    ceil(p/256) * ceil(q/256) = 4 workgroups without splitting K (9 ms per product, 70 % of a training step,
    profiles/r02_train_kernel_stats.csv); here it is the split-K fp32-MFMA GEMM of the C ABI, K cut over
    the chip and the slabs added in a fixed order (deterministic)."""

    @staticmethod
    def forward(ctx, A, B):
        lib = _lib.load()
        A, B = A.contiguous(), B.contiguous()
        n, p = A.shape
        q = B.shape[1]
        dev = A.device
        C_ = torch.empty((p, q), dtype=torch.float32, device=dev)
        splits = _splits_for(p, q, n)
        with torch.cuda.device(dev):
            skw = torch.empty(max(256, lib.rtk_gemm_f32_splitk_workspace_bytes(p, q, splits)), dtype=torch.uint8, device=dev)
            _lib.check(lib.rtk_gemm_f32_splitk(A.data_ptr(), 0, p, B.data_ptr(), 0, q, C_.data_ptr(), q, p, q, n, splits,
                                               skw.data_ptr(), skw.numel(), _stream_ptr(dev)), "rtk_gemm_f32_splitk (A^T B)")
        ctx.save_for_backward(A, B)
        return C_

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        dA = B @ dC.transpose(0, 1) if ctx.needs_input_grad[0] else None      # (n, q) @ (q, p): n row blocks, fills the chip
        dB = A @ dC if ctx.needs_input_grad[1] else None
        return dA, dB


def gram_tn(A, B):
    """``A.T @ B``; tall-skinny fp32 GPU operands go through the split-K HIP GEMM, anything else through torch
    (the Riemannian layer is generic torch code: float64 CPU tensors in its tests)."""
    if (A.is_cuda and A.dtype == torch.float32 and B.dtype == torch.float32 and A.dim() == 2 and B.dim() == 2
            and A.shape[0] == B.shape[0] and A.shape[0] >= 8192 and A.shape[0] >= 8 * max(A.shape[1], B.shape[1])):
        return _GramTN.apply(A, B)
    return A.transpose(0, 1) @ B


# What the two losses on a stored (B, N) matrix differ in: the public name, what the score kernel stores (with or without
# the logistic), the entries of the row sums and of the in-place gradient, and ``softmax``: the mean is taken over the B
# rows (not the B N entries), whose log-sum-exp the rows entry hands to the gradient entry.
_StoredLoss = collections.namedtuple("_StoredLoss", "who stored sigmoid rows grad softmax")
_STORED_BCE = _StoredLoss("bce_loss_1vN", "scores", True, "rtk_bce_rows_f32", "rtk_bce_grad_f32", False)
_STORED_CE = _StoredLoss("ce_loss_1vN", "logits", False, "rtk_ce_rows_f32", "rtk_ce_grad_f32", True)


def _stored_loss_forward(ctx, kind, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, eps):
    """The matrix (scores or logits) on aligned rows -- it never leaves the function pair --, its row sums, their mean."""
    ctx.kind, ctx.eps, ctx.B = kind, float(eps), int(subject_idx.numel())
    if ctx.B == 0:
        ctx.save_for_backward(core, R, S, O)
        return torch.zeros((), dtype=torch.float32, device=core.device)
    M, v, op = _forward(core, R, S, O, subject_idx, relation_idx, kind.sigmoid, False, want_v=True, padded=True)
    dev = M.device
    B, N = M.shape
    ctx.count = B if kind.softmax else B * N
    ctx.ld = _ld(M) if kind.softmax else M.stride(0)      # (the BCE pair has always been given the buffer's pitch at B = 1 too)
    rows = torch.empty(B, dtype=torch.float64, device=dev)
    lse = (torch.empty(B, dtype=torch.float32, device=dev),) if kind.softmax else ()
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), kind.rows)(M.data_ptr(), B, N, ctx.ld, pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                   pair_obj.data_ptr(), ctx.eps, rows.data_ptr(),
                                                   *(t.data_ptr() for t in lse), _stream_ptr(dev)), kind.rows)
    ctx.save_for_backward(op.core, op.R, op.S, op.O, op.h, op.r, v, M, pair_slot, pair_ptr, pair_obj, *lse)
    return (rows.sum() / ctx.count).to(torch.float32)


def _stored_loss_backward(ctx, grad_loss):
    """In place ``M <- d loss / d logits`` (the saved matrix is spent), then the gradient tail."""
    if ctx.B == 0:
        return _zero_batch_grads(ctx)
    core, R, S, O, h, r, v, M, pair_slot, pair_ptr, pair_obj, *lse = ctx.saved_tensors
    kind, norm = ctx.kind, 1.0 / ctx.count
    _spend(ctx, kind.who, kind.stored)
    dev = M.device
    B, N = M.shape
    g = grad_loss.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    with torch.cuda.device(dev):
        # BCE: M <- (P - y) g / (B N); CE: M <- (w softmax - y) g / B
        _lib.check(getattr(_lib.load(), kind.grad)(M.data_ptr(), B, N, ctx.ld, pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                   pair_obj.data_ptr(), ctx.eps, *(t.data_ptr() for t in lse), g.data_ptr(),
                                                   norm, _stream_ptr(dev)), kind.grad)
    # |dZ| <= |g| norm (|P - y| <= 1, |w softmax - y| <= 1): the operand bound of the split-fp16 GEMMs, no pass over dZ
    return _grads_from_dZ(core, R, S, O, h, r, v, M, ctx.needs_input_grad, dz_bound=g.abs() * norm) + (None,) * 6


class _BceLoss1vN(torch.autograd.Function):
    """mean BCE(sigmoid(logits), smoothed multi-hot targets) with the targets given as a CSR."""

    @staticmethod
    def forward(ctx, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, label_smoothing):
        ctx.fused = False
        if (FUSED_BCE and core.dtype == torch.float32 and core.is_cuda and _packed_stage2(core.shape[2], exact=False)
                and core.shape[1] == core.shape[2] and subject_idx.numel() > 0):
            return _BceLoss1vN._forward_fused(ctx, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj,
                                              float(label_smoothing))
        return _stored_loss_forward(ctx, _STORED_BCE, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj,
                                    label_smoothing)

    @staticmethod
    def _forward_fused(ctx, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, eps):
        """Loss fused into the score kernel's epilogue (``rtk_score_packed_bce_f32``): the B x N matrix is written once,
        as ``x = p - eps / N`` (the logit gradient of a negative, up to g / (B N)), never re-read in the forward; the few
        positives are patched by ``rtk_bce_patch_pos_f32``."""
        lib = _lib.load()
        op = _Operands(core, R, S, O, subject_idx, relation_idx)
        B, N, c, dev = op.B, op.O.shape[0], op.c, op.dev
        v = torch.empty((B, c), dtype=torch.float32, device=dev)
        X = alloc_scores(B, N, dev)
        partials = torch.empty(lib.rtk_score_bce_partials(), dtype=torch.float64, device=dev)
        rows_pos = torch.empty(4 * B, dtype=torch.float64, device=dev)      # four partial sums per row
        ld = _ld(X)
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            qp = _packed_buffer(dev, sp, _size("rtk_packed_query_bytes", op.dcode, B, c))
            _strict_check(_stage1(op, sp, None, v, qp), sp)
            _lib.check(lib.rtk_score_packed_bce_f32(qp.data_ptr(), B, c, op.O.data_ptr(), N, X.data_ptr(), ld, eps,
                                                    partials.data_ptr(), sp), "rtk_score_packed_bce_f32")
            _lib.check(lib.rtk_bce_patch_pos_f32(X.data_ptr(), B, N, ld, pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                 pair_obj.data_ptr(), eps, v.data_ptr(), op.O.data_ptr(), c,
                                                 rows_pos.data_ptr(), sp), "rtk_bce_patch_pos_f32")
        ctx.save_for_backward(op.core, op.R, op.S, op.O, op.h, op.r, v, X, pair_slot, pair_ptr, pair_obj)
        ctx.eps = eps
        ctx.fused = True
        return ((partials.sum() + rows_pos.sum()) / (B * N)).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_loss):
        if not ctx.fused:
            return _stored_loss_backward(ctx, grad_loss)
        core, R, S, O, h, r, v, X = ctx.saved_tensors[:8]
        B, N = X.shape
        g = grad_loss.to(device=X.device, dtype=torch.float32).reshape(1) * (1.0 / (B * N))
        # X = (p - y) unscaled, |X| <= 1: the GEMMs' operand bound; g / (B N) rides on the small operands
        return _grads_from_dZ(core, R, S, O, h, r, v, X, ctx.needs_input_grad,
                              dz_bound=torch.ones(1, dtype=torch.float32, device=X.device), scale=g) + (None,) * 6


# Largest object rank of the matrix-free loss (rtk_bce_stream_*: one wave keeps a whole row of the dv / gO accumulator).
_STREAM_MAX_C = 208


def _csr_slots(flt, item_ids, dev, max_pos=0):
    """``(pair_slot, max_pos)``: the filter's CSR slot of every item of the batch, and the bound on the CSR entries of its
    queries, for ``max_pos=None`` ``B * flt.max_list``, which always holds (a filter without ``max_list``: all it has)."""
    slot = flt.slot_of_item[item_ids.to(dev)].contiguous()
    if max_pos is None:
        mx = getattr(flt, "max_list", None)
        max_pos = int(slot.numel()) * int(mx) if mx is not None else int(flt.pair_obj.numel())
    return slot, int(max_pos)


def bce_loss_1vN(core, R, S, O, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0, matrix_free=False,
                 sigmoid_mode=None, max_pos=None):
    """The reference's training loss term ``nn.BCELoss()(score_fn(T), targets)`` (train.py:79,136) for a
    batch of (subject, relation) items WITHOUT the dense target matrix: ``flt`` is the
    ``evaluation.DeviceFilter`` of the train-mode ``KG_dataset`` (CSR of known objects per pair, on
    the device), ``item_ids`` the dataset indices of the batch; the targets
    ``(1 - eps) * multi_hot + eps / N`` (Dataset.py:51-52) are applied inside the kernels.
    Differentiable w.r.t. core and factors like ``score_1vN``.

    ``matrix_free=True``: the same loss and gradients without the (B, N) matrix (``rtk_bce_stream_*``): nothing that
    grows with B x N is allocated in forward, backward or between them.  float32 operands with ``c <= 208``,
    ``c % 4 == 0`` (anything else raises; there is no fallback; bf16 operands up to ``c = 512`` are served by
    ``bce_loss_block_1vN`` on the whole range and by ``ShardedEntityScorer.bce_loss_1vN``).  ``sigmoid_mode`` ("fast" / "exact", default
    ``DEFAULT_SIGMOID``) applies to this form only; the probabilities are the ws score kernel's.  ``max_pos``: an upper
    bound on the number of CSR entries of the batch's queries (default ``B * flt.max_list``, which always holds)."""
    if matrix_free:                      # the whole matrix is one block: col0 = 0, n_ent = N, nothing to reduce
        return _block_loss(_HipBlockLoss, core, R, S, O, 0, O.shape[0], subject_idx, relation_idx, flt, item_ids,
                           label_smoothing, sigmoid_mode, max_pos, None, who="bce_loss_1vN(matrix_free=True)")
    if sigmoid_mode is not None or max_pos is not None:
        raise ValueError("sigmoid_mode and max_pos belong to matrix_free=True")
    slot, _ = _csr_slots(flt, item_ids, core.device)
    return _BceLoss1vN.apply(core, R, S, O, subject_idx, relation_idx, slot, flt.pair_ptr, flt.pair_obj,
                             float(label_smoothing))


class _HipBlockLoss:
    """The device steps of the block loss (``rtk_bce_stream_*_part_f32`` around stage 1 and its backward).
    ``ShardedEntityScorer.bce_loss_1vN`` lets tests put CPU functions with these signatures in their place."""

    @staticmethod
    def operands(core, R, S, O_loc, subject_idx, relation_idx, col0, n_ent, who):
        """The checked, contiguous operands ``(core, R, S, O_loc, h, r)``; the refusals of ``matrix_free=True``, under
        the name ``who`` of the public function that was called."""
        _require_gpu("core", core)
        if core.dtype != torch.float32:
            served = ("the matrix form, or bce_loss_block_1vN / ShardedEntityScorer.bce_loss_1vN on the whole range"
                      if who.startswith("bce_loss_1vN") else "the matrix form")
            raise RuntimeError(f"{who}: float32 operands only, got {core.dtype} (bf16 operands: {served})")
        op = _Operands(core, R, S, O_loc, subject_idx, relation_idx)
        n_local, c = op.O.shape
        if c > _STREAM_MAX_C or c % 4 != 0 or op.O.data_ptr() % 16 != 0:
            raise RuntimeError(f"{who}: object rank c = {c} outside the matrix-free range "
                               f"(c <= {_STREAM_MAX_C}, c % 4 == 0, 16-byte-aligned O)")
        if col0 < 0 or n_ent < 1 or col0 + n_local > n_ent:
            raise RuntimeError(f"{who}: block [{col0}, {col0} + {n_local}) is not a part of [0, n_ent = {n_ent})")
        return op.core, op.R, op.S, op.O, op.h, op.r

    @staticmethod
    def queries(core, R, S, h, r):
        """Stage 1 of all B queries: the fp32 query vectors and their packed planes."""
        op = _Operands(core, R, S, None, h, r)
        v = torch.empty((op.B, op.c), dtype=torch.float32, device=op.dev)
        qp = torch.empty(_size("rtk_packed_query_bytes", op.dcode, op.B, op.c), dtype=torch.uint8, device=op.dev)
        with torch.cuda.device(op.dev):
            sp = _stream_ptr(op.dev)
            _strict_check(_stage1(op, sp, None, v, qp), sp)
        return v, qp

    @staticmethod
    def rows(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, eps, sigmoid_mode, want_dv):
        """Sweep 1 on the block: ``(rows float64 (B,), dv float32 (B, c) or None)``, the block's shares."""
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        flags = _score_flags(True, sigmoid_mode, torch.float32, False)
        rows = torch.empty(B, dtype=torch.float64, device=dev)
        dv = torch.empty((B, c), dtype=torch.float32, device=dev) if want_dv else None
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_bce_stream_part_workspace_bytes", B, n_local, c, 0))
            _lib.check(lib.rtk_bce_stream_rows_part_f32(qp.data_ptr(), B, c, O_loc.data_ptr(), n_local, col0, n_ent,
                                                        pair_slot.data_ptr(), pair_ptr.data_ptr(), pair_obj.data_ptr(),
                                                        eps, flags, rows.data_ptr(), dv.data_ptr() if want_dv else None,
                                                        ws.data_ptr(), ws.numel(), sp), "rtk_bce_stream_rows_part_f32")
        return rows, dv

    @staticmethod
    def grad_o(qp, v, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps, sigmoid_mode, scale):
        """Sweep 2 on the block: its rows of gO, ``scale`` (one float on the device) = g / (B n_ent)."""
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        flags = _score_flags(True, sigmoid_mode, torch.float32, False)
        gO = torch.empty((n_local, c), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_bce_stream_part_workspace_bytes", B, n_local, c, max_pos))
            _lib.check(lib.rtk_bce_stream_grad_o_part_f32(qp.data_ptr(), v.data_ptr(), B, c, O_loc.data_ptr(), n_local, col0,
                                                          n_ent, pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                          pair_obj.data_ptr(), max_pos, eps, flags, scale.data_ptr(),
                                                          gO.data_ptr(), ws.data_ptr(), ws.numel(), sp),
                       "rtk_bce_stream_grad_o_part_f32")
            _strict_check(ws, sp)
        return gO

    @staticmethod
    def stage1_backward(core, R, S, h, r, dv, needs):
        """``(g_core, g_R, g_S)`` from the scaled dv."""
        return _stage1_backward(core, R, S, h, r, dv, needs)


# Largest object rank of the matrix-free BCE loss on bf16 operands (rtk_bce_stream_*_part_bf16: the second tile product of
# both sweeps is cut into chunks of 128 output columns).
_STREAM_MAX_C_BF16 = 512
# The fp32 rows of gO that sweep 2 writes per call on bf16 operands: the gradient is returned in bf16, so the block's rows
# go through an fp32 staging buffer of at most this size, a sub-block of rows per call, instead of a whole fp32 gO
# beside its bf16 copy.
_GO_STAGE_BYTES = 32 << 20


class _HipBlockLossAnyDtype(_HipBlockLoss):
    """``_HipBlockLoss`` for float32 OR bfloat16 operands: the steps of ``bce_loss_block_1vN`` and
    ``ShardedEntityScorer.bce_loss_1vN``.  With bf16 operands stage 1 runs on them as given, the sweeps are
    ``rtk_bce_stream_*_part_bf16`` (no fp32 copy of ``O_loc``), the stage-1 backward runs on fp32 copies of core, R and S
    (small) on its gemm route and on the bf16 operands themselves on its stream route (``stage1_backward_route``), and
    every gradient comes back in bf16, as the matrix form's do (``_grads_like``); the rows of gO go through
    an fp32 staging buffer of ``_GO_STAGE_BYTES``, a sub-block of rows per call.  The float32 path is the parent's, call
    for call."""

    @staticmethod
    def operands(core, R, S, O_loc, subject_idx, relation_idx, col0, n_ent, who):
        _require_gpu("core", core)
        if core.dtype != torch.bfloat16:
            return _HipBlockLoss.operands(core, R, S, O_loc, subject_idx, relation_idx, col0, n_ent, who)
        op = _Operands(core, R, S, O_loc, subject_idx, relation_idx)      # one dtype for all four: mixed ones are refused
        n_local, c = op.O.shape
        if c > _STREAM_MAX_C_BF16 or c % 8 != 0 or op.O.data_ptr() % 16 != 0:
            raise RuntimeError(f"{who}: object rank c = {c} outside the matrix-free range of bf16 operands "
                               f"(c <= {_STREAM_MAX_C_BF16}, c % 8 == 0, 16-byte-aligned O)")
        if col0 < 0 or n_ent < 1 or col0 + n_local > n_ent:
            raise RuntimeError(f"{who}: block [{col0}, {col0} + {n_local}) is not a part of [0, n_ent = {n_ent})")
        return op.core, op.R, op.S, op.O, op.h, op.r

    @staticmethod
    def rows(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, eps, sigmoid_mode, want_dv):
        if O_loc.dtype != torch.bfloat16:
            return _HipBlockLoss.rows(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, eps, sigmoid_mode, want_dv)
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        flags = _score_flags(True, sigmoid_mode, torch.float32, True)
        rows = torch.empty(B, dtype=torch.float64, device=dev)
        dv = torch.empty((B, c), dtype=torch.float32, device=dev) if want_dv else None
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_bce_stream_bf16_workspace_bytes", B, n_local, c, 0))
            _lib.check(lib.rtk_bce_stream_rows_part_bf16(qp.data_ptr(), B, c, O_loc.data_ptr(), n_local, col0, n_ent,
                                                         pair_slot.data_ptr(), pair_ptr.data_ptr(), pair_obj.data_ptr(),
                                                         eps, flags, rows.data_ptr(), dv.data_ptr() if want_dv else None,
                                                         ws.data_ptr(), ws.numel(), sp), "rtk_bce_stream_rows_part_bf16")
        return rows, dv

    @staticmethod
    def grad_o(qp, v, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps, sigmoid_mode, scale):
        if O_loc.dtype != torch.bfloat16:
            return _HipBlockLoss.grad_o(qp, v, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps,
                                        sigmoid_mode, scale)
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        flags = _score_flags(True, sigmoid_mode, torch.float32, True)
        gO = torch.empty((n_local, c), dtype=torch.bfloat16, device=dev)
        # whole 128-row entity tiles per call; a sub-block of a block is a block (rows [col0 + lo, col0 + hi) of n_ent)
        step = min(n_local, max(128, _GO_STAGE_BYTES // (4 * c) // 128 * 128))
        stage = torch.empty((step, c), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_bce_stream_bf16_workspace_bytes", B, step, c, max_pos))
            for lo in range(0, n_local, step):
                n = min(step, n_local - lo)
                _lib.check(lib.rtk_bce_stream_grad_o_part_bf16(qp.data_ptr(), v.data_ptr(), B, c,
                                                               O_loc.data_ptr() + 2 * lo * c, n, col0 + lo, n_ent,
                                                               pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                               pair_obj.data_ptr(), max_pos, eps, flags, scale.data_ptr(),
                                                               stage.data_ptr(), ws.data_ptr(), ws.numel(), sp),
                           "rtk_bce_stream_grad_o_part_bf16")
                gO[lo:lo + n].copy_(stage[:n])
            _strict_check(ws, sp)
        return gO

    @staticmethod
    def stage1_backward(core, R, S, h, r, dv, needs):
        return _grads_like(_stage1_backward(core, R, S, h, r, dv, needs), core.dtype)


def _block_enter(ctx, steps, core, R, S, O_loc, subject_idx, relation_idx, eps, max_pos, col0, n_ent, all_reduce, who):
    """What the forwards of the two block losses begin with: the checked operands ``(core, R, S, O_loc, h, r)``, and on
    ``ctx`` what their backwards share.  -> ``(operands, zero)``; ``zero`` is the loss of an empty batch (None otherwise)."""
    operands = steps.operands(core, R, S, O_loc, subject_idx, relation_idx, col0, n_ent, who)
    core = operands[0]
    # float32 like the matrix forms; float64 stand-ins of the steps (tests on the CPU) keep their precision
    ctx.ldt = torch.float64 if core.dtype == torch.float64 else torch.float32
    ctx.eps, ctx.max_pos, ctx.B, ctx.dv_saved = float(eps), int(max_pos), operands[4].numel(), False
    ctx.col0, ctx.n_ent, ctx.all_reduce, ctx.steps = col0, n_ent, all_reduce, steps
    if ctx.B > 0:
        return operands, None
    ctx.save_for_backward(*operands[:4])
    return operands, torch.zeros((), dtype=ctx.ldt, device=core.device)


def _finish_dv(ctx, dv, g, needs):
    """``(g_core, g_R, g_S)`` from a block's unscaled dv: dv, (B, c), never gS, (n_ent, b), is summed over the ranks (on
    a copy where it is the forward's saved share, which stays as it is), then ``g`` and the (linear) stage-1 backward."""
    if not any(needs[:3]):
        return None, None, None
    core, R, S, _, h, r = ctx.saved_tensors[:6]
    if ctx.all_reduce is not None:
        dv = dv.clone() if ctx.dv_saved else dv
        ctx.all_reduce(dv)
    return tuple(ctx.steps.stage1_backward(core, R, S, h, r, dv * g, needs))


class _BceLossBlock(torch.autograd.Function):
    """``_BceLoss1vN`` without the score matrix (``rtk_bce_stream_*_part_f32``), on rows ``[col0, col0 + n_local)`` of the
    entity matrix: sweep 1 (loss rows and dv) in the forward, sweep 2 (gO) in the backward.  What is saved is of size
    B x c: the fp32 query vectors, their packed planes, dv.  The whole matrix is the block ``col0 = 0, n_ent = N``.
    Without ``all_reduce`` the block's share of the loss and of the gradients of core, R, S; with it the loss rows are
    summed over the ranks in the forward and dv in the backward, before the (linear) stage-1 backward.  The gradient of
    ``O_loc`` is always local.  ``who``: the public function's name, for the refusals."""

    @staticmethod
    def forward(ctx, core, R, S, O_loc, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, eps, sigmoid_mode, max_pos,
                want_dv, col0, n_ent, all_reduce, steps, who="bce_loss_block_1vN"):
        (core, R, S, O_loc, h, r), zero = _block_enter(ctx, steps, core, R, S, O_loc, subject_idx, relation_idx, eps, max_pos,
                                                       col0, n_ent, all_reduce, who)
        if zero is not None:
            return zero
        ctx.mode, ctx.who, ctx.dv_saved = sigmoid_mode, who, want_dv
        B, (n_local, c), dev, ldt = ctx.B, O_loc.shape, core.device, ctx.ldt
        v = qp = None
        if n_local > 0:
            v, qp = steps.queries(core, R, S, h, r)
            rows, dv = steps.rows(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, ctx.eps, sigmoid_mode, want_dv)
        else:                                    # a rank without rows adds nothing and still takes part in the sums
            rows = torch.zeros(B, dtype=torch.float64, device=dev)
            dv = torch.zeros((B, c), dtype=ldt, device=dev) if want_dv else None
        if all_reduce is not None:
            all_reduce(rows)
        ctx.save_for_backward(core, R, S, O_loc, h, r, v, qp, pair_slot, pair_ptr, pair_obj, dv)
        return (rows.sum() / (B * n_ent)).to(ldt)

    @staticmethod
    def backward(ctx, grad_loss):
        needs = ctx.needs_input_grad
        if ctx.B == 0:
            return _zero_batch_grads(ctx)
        _, _, _, O_loc, _, _, v, qp, pair_slot, pair_ptr, pair_obj, dv = ctx.saved_tensors
        B = ctx.B
        g = (grad_loss.to(device=O_loc.device, dtype=ctx.ldt).reshape(1) * (1.0 / (B * ctx.n_ent))).contiguous()
        gO = None
        if needs[3]:
            gO = (ctx.steps.grad_o(qp, v, B, O_loc, ctx.col0, ctx.n_ent, pair_slot, pair_ptr, pair_obj, ctx.max_pos, ctx.eps,
                                   ctx.mode, g) if O_loc.shape[0] > 0 else torch.zeros_like(O_loc))
        if any(needs[:3]) and not ctx.dv_saved:
            raise RuntimeError(f"{ctx.who}: dv was not computed in the forward")
        return _finish_dv(ctx, dv, g, needs) + (gO,) + (None,) * 14


def _block_loss(steps, core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids, label_smoothing,
                sigmoid_mode, max_pos, all_reduce, who="bce_loss_block_1vN"):
    slot, max_pos = _csr_slots(flt, item_ids, core.device, max_pos)
    # dv (the second tile product of sweep 1) only when a gradient of core, R or S can be asked for
    want_dv = _wants_grad(core, R, S)
    return _BceLossBlock.apply(core, R, S, O_loc, subject_idx, relation_idx, slot, flt.pair_ptr, flt.pair_obj,
                               float(label_smoothing), sigmoid_mode, max_pos, want_dv, int(col0), int(n_ent),
                               all_reduce, steps, who)


def bce_loss_block_1vN(core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0,
                       sigmoid_mode=None, max_pos=None, all_reduce=None):
    """``bce_loss_1vN(..., matrix_free=True)`` on one block of entity rows (an entity shard), without anything of size
    B x n_local (``rtk_bce_stream_rows_part_f32`` / ``rtk_bce_stream_grad_o_part_f32``).  ``O_loc``: rows
    ``[col0, col0 + n_local)`` of the (n_ent, c) entity matrix; ``flt`` holds GLOBAL entity ids; the smoothing term is
    ``eps / n_ent``.  S is only indexed by ``subject_idx`` and need not have n_ent rows.

    ``all_reduce=None``: the block's SHARE of the loss, ``rows.sum() / (B * n_ent)``; its backward gives the block's
    share of the gradients of core, R and S (the stage-1 backward is linear in dv) and the gradient of ``O_loc``.
    Summed over any partition of [0, n_ent) the shares are the loss and gradients of the whole matrix.

    ``all_reduce=fn`` (``fn(t)`` sums ``t`` in place over the ranks): the forward reduces the B float64 loss rows and
    returns the complete loss, equal on every rank; the backward reduces dv (B x c floats) before the stage-1
    backward, so core / R / S receive their complete gradients, identical on every rank -- do not average them again;
    ``O_loc.grad`` is local.  A block without rows contributes zeros and still calls ``fn``.

    float32 with ``c <= 208``, ``c % 4 == 0``, or bfloat16 (all four operands) with ``c <= 512``, ``c % 8 == 0``
    (``rtk_bce_stream_*_part_bf16``: the probabilities are the bf16 score kernel's, no fp32 copy of ``O_loc`` is made,
    the loss is float32 and the gradients come back in bf16 like the matrix form's); anything else raises, there is no
    fallback.  ``sigmoid_mode`` / ``max_pos`` / the ``index_check`` policy as ``bce_loss_1vN(matrix_free=True)``;
    ``max_pos`` bounds the CSR entries of the batch's queries in all blocks.  Under ``no_grad``, or when core, R and S
    want no gradient, dv is not computed."""
    _require_gpu("core", core)
    return _block_loss(_HipBlockLossAnyDtype, core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids,
                       label_smoothing, sigmoid_mode, max_pos, all_reduce)


class _CeLoss1vN(torch.autograd.Function):
    """mean softmax cross-entropy of the stored logits against the smoothed, per-row normalised targets given as a CSR
    (``rtk_ce_rows_f32`` / ``rtk_ce_grad_f32``): the matrix form, any object rank."""

    @staticmethod
    def forward(ctx, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, label_smoothing):
        return _stored_loss_forward(ctx, _STORED_CE, core, R, S, O, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj,
                                    label_smoothing)

    backward = staticmethod(_stored_loss_backward)


def ce_loss_1vN(core, R, S, O, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0, matrix_free=False,
                max_pos=None):
    """The softmax cross-entropy 1-vs-all loss over the entities, the other standard training loss of link prediction
    (what ``torch.nn.functional.cross_entropy(logits, y)`` with probability targets and mean reduction gives), WITHOUT
    the dense target matrix: ``flt`` and ``item_ids`` as for ``bce_loss_1vN``.  With ``P_d`` the filter's list of item
    d, ``n_d`` its length, N the entity count and eps the smoothing, the targets are
    ``y[d, j] = (1 - eps) [j in P_d] / n_d + eps / N`` (the first term absent for an empty list), of row mass
    ``w_d = (1 - eps) [n_d > 0] + eps``, and

        loss = (1 / B) sum_d (w_d logsumexp(z_d) - sum_j y[d, j] z[d, j]),
        d loss / d z[d, j] = (w_d softmax(z_d)_j - y[d, j]) / B.

    The loss does not depend on the level of a row's logits.  Differentiable w.r.t. core and factors like
    ``score_1vN``; a shared-factor model passes the same tensor as ``S`` and ``O``.

    ``matrix_free=False``: on the stored logits of ``score_1vN(sigmoid=False)`` (``rtk_ce_rows_f32`` /
    ``rtk_ce_grad_f32``), float32 operands at any object rank; one backward per forward.
    ``matrix_free=True``: the same loss and gradients without the (B, N) matrix, as ``ce_loss_block_1vN`` on the whole
    range (``rtk_ce_stream_rows_part_f32`` / ``rtk_ce_stream_grad_part_f32`` at ``col0 = 0``, the logarithm taken on
    the B float64 sums): what is kept between forward and backward is B x c and B.  float32 operands with
    ``c <= 208``, ``c % 4 == 0`` (anything else raises; there is no fallback).  Under ``no_grad`` only the forward sweep
    runs.  ``max_pos``: an upper bound on the number of CSR entries of the batch's queries (default
    ``B * flt.max_list``, which always holds)."""
    _require_gpu("core", core)
    if matrix_free:                      # the whole matrix is one block: col0 = 0, n_ent = N, nothing to exchange
        return _ce_block_loss(_HipCeBlockLoss, core, R, S, O, 0, O.shape[0], subject_idx, relation_idx, flt, item_ids,
                              label_smoothing, max_pos, None, None, None, who="ce_loss_1vN(matrix_free=True)")
    if max_pos is not None:
        raise ValueError("max_pos belongs to matrix_free=True")
    if core.dtype != torch.float32:
        raise RuntimeError(f"ce_loss_1vN: float32 operands only, got {core.dtype}")
    slot, _ = _csr_slots(flt, item_ids, core.device)
    return _CeLoss1vN.apply(core, R, S, O, subject_idx, relation_idx, slot, flt.pair_ptr, flt.pair_obj,
                            float(label_smoothing))


class _HipCeBlockLoss(_HipBlockLoss):
    """The device steps of the cross-entropy block loss: ``operands``, ``queries`` and ``stage1_backward`` of the BCE
    steps, with ``rtk_ce_stream_*_part_f32`` between them.  ``ShardedEntityScorer.ce_loss_1vN`` lets tests put CPU
    functions with these signatures in their place."""

    @staticmethod
    def partials(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, eps):
        """The forward sweep on the block: ``(m float32 (B,), s float64 (B,), lin float64 (B,))``."""
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        m = torch.empty(B, dtype=torch.float32, device=dev)
        s = torch.empty(B, dtype=torch.float64, device=dev)
        lin = torch.empty(B, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_ce_stream_part_workspace_bytes", B, n_local, c, 0))
            _lib.check(lib.rtk_ce_stream_rows_part_f32(qp.data_ptr(), B, c, O_loc.data_ptr(), n_local, col0, n_ent,
                                                       pair_slot.data_ptr(), pair_ptr.data_ptr(), pair_obj.data_ptr(), eps,
                                                       m.data_ptr(), s.data_ptr(), lin.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       sp), "rtk_ce_stream_rows_part_f32")
        return m, s, lin

    @staticmethod
    def grad(qp, v, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps, lse, scale, want_dv, want_gO):
        """The two backward sweeps on the block from the GLOBAL ``lse`` (float64 (B,), cast to float32 here):
        ``(dv float32 (B, c) or None, gO float32 (n_local, c) or None)``; dv is the block's unscaled share, gO carries
        ``scale`` (one float on the device) = g / B."""
        lib = _lib.load()
        dev = O_loc.device
        n_local, c = O_loc.shape
        lse32 = lse.to(torch.float32).contiguous()
        dv = torch.empty((B, c), dtype=torch.float32, device=dev) if want_dv else None
        gO = torch.empty((n_local, c), dtype=torch.float32, device=dev) if want_gO else None
        if not (want_dv or want_gO):
            return dv, gO
        max_pos = max_pos if want_gO else 0
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            ws = _workspace(dev, sp, _size("rtk_ce_stream_part_workspace_bytes", B, n_local, c, max_pos))
            _lib.check(lib.rtk_ce_stream_grad_part_f32(qp.data_ptr(), v.data_ptr(), B, c, O_loc.data_ptr(), n_local, col0,
                                                       n_ent, pair_slot.data_ptr(), pair_ptr.data_ptr(),
                                                       pair_obj.data_ptr(), max_pos, eps, lse32.data_ptr(), scale.data_ptr(),
                                                       dv.data_ptr() if want_dv else None,
                                                       gO.data_ptr() if want_gO else None, ws.data_ptr(), ws.numel(), sp),
                       "rtk_ce_stream_grad_part_f32")
            _strict_check(ws, sp)
        return dv, gO


def _ce_row_mass(pair_slot, pair_ptr, eps):
    """w_d = (1 - eps) [n_d > 0] + eps in float64, n_d the STORED list length (0 for pair_slot[d] < 0)."""
    ends = pair_ptr.unfold(0, 2, 1)[pair_slot.clamp(min=0)]      # (B, 2), one gather: where each list begins and ends
    has = (ends[:, 1] > ends[:, 0]) & (pair_slot >= 0)
    return has.to(torch.float64) * (1.0 - eps) + eps


def _ce_empty_partials(B, dev, mdt=torch.float32):
    """What a block without rows contributes: m = -inf, s = 0, lin = 0."""
    return (torch.full((B,), float("-inf"), dtype=mdt, device=dev),
            torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev))


class _CeLossBlock(torch.autograd.Function):
    """``_CeLoss1vN`` without the logit matrix (``rtk_ce_stream_*_part_f32``), on rows ``[col0, col0 + n_local)`` of the
    entity matrix: one sweep in the forward, two (dv, gO) in the backward.  The whole matrix is the block ``col0 = 0,
    n_ent = N``.  The row's log-sum-exp couples the blocks, so the forward gives the block's ``(m, s, lin)`` and one of
    three things completes it: the two collectives (MAX of m, SUM of ``[s exp(m - M), lin]``), a given global ``lse``
    (the block's share, no collectives) or nothing (the block is the whole range).  The backward is ``grad_part`` with
    the global lse; with ``all_reduce`` dv is summed over the ranks before the (linear) stage-1 backward.  The gradient
    of ``O_loc`` is always local.  What is saved is of size B x c and B."""

    @staticmethod
    def forward(ctx, core, R, S, O_loc, subject_idx, relation_idx, pair_slot, pair_ptr, pair_obj, eps, max_pos, col0, n_ent,
                all_reduce, all_reduce_max, lse, steps, who="ce_loss_block_1vN"):
        (core, R, S, O_loc, h, r), zero = _block_enter(ctx, steps, core, R, S, O_loc, subject_idx, relation_idx, eps, max_pos,
                                                       col0, n_ent, all_reduce, who)
        if zero is not None:
            return zero
        B, (n_local, c), dev, ldt = ctx.B, O_loc.shape, core.device, ctx.ldt
        v = qp = None
        if n_local > 0:
            v, qp = steps.queries(core, R, S, h, r)
            m, s, lin = steps.partials(qp, B, O_loc, col0, n_ent, pair_slot, pair_ptr, pair_obj, ctx.eps)
        else:                                    # a rank without rows adds nothing and still takes part in the exchanges
            m, s, lin = _ce_empty_partials(B, dev, ldt)
        # (the kernels form w, t0 and 1 - eps from the float32 eps they are given)
        w = _ce_row_mass(pair_slot, pair_ptr, ctx.eps if ldt == torch.float64 else torch.tensor(ctx.eps, dtype=ldt).item())
        if all_reduce is not None:              # MAX of B floats, then SUM of (2, B) doubles
            M = m.clone()
            all_reduce_max(M)
            M = M.to(torch.float64)
            t = torch.stack([s * torch.exp(m.to(torch.float64) - M), lin])
            all_reduce(t)
            lse = M + torch.log(t[0])
            rows = w * lse + t[1]
        elif lse is not None:                    # the block's share: its softmax mass of w lse, and its linear part
            sigma = s * torch.exp(m.to(torch.float64) - lse)
            rows = w * lse * sigma + lin
        else:                                    # the whole range
            lse = torch.log(s).add_(m)          # float64: m is converted inside the sum
            rows = w * lse + lin
        ctx.save_for_backward(core, R, S, O_loc, h, r, v, qp, lse, pair_slot, pair_ptr, pair_obj)
        return (rows.sum() / B).to(ldt)

    @staticmethod
    def backward(ctx, grad_loss):
        needs = ctx.needs_input_grad
        if ctx.B == 0:
            return _zero_batch_grads(ctx)
        _, _, _, O_loc, _, _, v, qp, lse, pair_slot, pair_ptr, pair_obj = ctx.saved_tensors
        B, dev = ctx.B, O_loc.device
        n_local, c = O_loc.shape
        g = (grad_loss.to(device=dev, dtype=ctx.ldt).reshape(1) * (1.0 / B)).contiguous()
        want_dv = any(needs[:3])
        if n_local > 0:
            dv, gO = ctx.steps.grad(qp, v, B, O_loc, ctx.col0, ctx.n_ent, pair_slot, pair_ptr, pair_obj, ctx.max_pos,
                                    ctx.eps, lse, g, want_dv, bool(needs[3]))
        else:
            dv = torch.zeros((B, c), dtype=ctx.ldt, device=dev) if want_dv else None
            gO = torch.zeros_like(O_loc) if needs[3] else None
        return _finish_dv(ctx, dv, g, needs) + (gO,) + (None,) * 14


def _ce_block_loss(steps, core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids, label_smoothing,
                   max_pos, all_reduce, all_reduce_max, lse, who="ce_loss_block_1vN"):
    col0, n_ent, n_local = int(col0), int(n_ent), int(O_loc.shape[0])
    if (all_reduce is None) != (all_reduce_max is None):
        raise ValueError(f"{who}: all_reduce (SUM) and all_reduce_max (MAX) come together: the forward needs both")
    if lse is not None and all_reduce is not None:
        raise ValueError(f"{who}: lse= (the block's share, no exchange) and the collectives exclude each other")
    if lse is not None:
        B = int(subject_idx.numel())
        if not isinstance(lse, torch.Tensor) or lse.dtype != torch.float64 or tuple(lse.shape) != (B,):
            raise ValueError(f"{who}: lse must be the global log-sum-exp as a float64 tensor of shape ({B},)")
        lse = lse.detach().to(core.device).contiguous()
    elif all_reduce is None and not (col0 == 0 and n_local == n_ent):
        raise ValueError(f"{who}: block [{col0}, {col0} + {n_local}) of n_ent = {n_ent} without collectives or lse=: the "
                         "block's own log-sum-exp is not the loss")
    slot, max_pos = _csr_slots(flt, item_ids, core.device, max_pos)
    return _CeLossBlock.apply(core, R, S, O_loc, subject_idx, relation_idx, slot, flt.pair_ptr, flt.pair_obj,
                              float(label_smoothing), max_pos, col0, n_ent, all_reduce, all_reduce_max, lse, steps, who)


def ce_partials_block_1vN(core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0):
    """The forward of ``ce_loss_1vN(matrix_free=True)`` on one block of entity rows, stopped before the logarithm
    (stage 1 + ``rtk_ce_stream_rows_part_f32``; runs without grad): per query d and over the block's rows
    ``[col0, col0 + n_local)`` only, ``m`` (float32) the largest logit, ``s`` (float64) ``sum_j exp(z_j - m)`` and
    ``lin`` (float64) ``-eps / n_ent sum_j z_j - (1 - eps) / n_d sum_{t in P_d, t in block} z_t`` with the GLOBAL entity
    count and list length.  ``ce_merge_lse`` turns the blocks' ``(m, s)`` into the global lse; the loss rows are
    ``w_d lse_d + sum_k lin_k``.  A block without rows gives ``m = -inf, s = 0, lin = 0``."""
    _require_gpu("core", core)
    with torch.no_grad():
        who = "ce_partials_block_1vN"
        core, R, S, O_loc, h, r = _HipBlockLoss.operands(core, R, S, O_loc, subject_idx, relation_idx, int(col0), int(n_ent),
                                                         who)
        B = h.numel()
        if B == 0 or O_loc.shape[0] == 0:
            return _ce_empty_partials(B, core.device)
        slot, _ = _csr_slots(flt, item_ids, core.device)
        _, qp = _HipBlockLoss.queries(core, R, S, h, r)
        return _HipCeBlockLoss.partials(qp, B, O_loc, int(col0), int(n_ent), slot, flt.pair_ptr, flt.pair_obj,
                                        float(label_smoothing))


def ce_merge_lse(ms, ss):
    """The global log-sum-exp, float64 (B,), from the blocks' maxima ``ms`` and sums of exponentials ``ss`` (lists of
    ``ce_partials_block_1vN``'s ``m`` and ``s`` over a partition of the entities): ``M = max_k m_k``,
    ``lse = M + log sum_k s_k exp(m_k - M)``, all in float64.  A block without rows has ``m = -inf, s = 0``."""
    if len(ms) == 0 or len(ms) != len(ss):
        raise ValueError("ce_merge_lse: one m and one s per block, at least one block")
    m = torch.stack([t.to(torch.float64) for t in ms])
    s = torch.stack([t.to(torch.float64) for t in ss])
    M = m.max(dim=0).values
    return M + torch.log((s * torch.exp(m - M)).sum(dim=0))


def ce_loss_block_1vN(core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0,
                      max_pos=None, all_reduce=None, all_reduce_max=None, lse=None):
    """``ce_loss_1vN(..., matrix_free=True)`` on one block of entity rows (an entity shard), without anything of size
    B x n_local (``rtk_ce_stream_rows_part_f32`` / ``rtk_ce_stream_grad_part_f32``).  ``O_loc``: rows
    ``[col0, col0 + n_local)`` of the (n_ent, c) entity matrix; ``flt`` holds GLOBAL entity ids; the smoothing term is
    ``eps / n_ent`` and ``n_d`` the whole list's length.  S is only indexed by ``subject_idx`` and need not have n_ent
    rows.  Unlike the BCE loss this one is not a sum over entities: the row's log-sum-exp couples the blocks, so a
    block on its own gives ``(m, s, lin)`` (see ``ce_partials_block_1vN``) and needs one of the following.

    ``all_reduce=fn, all_reduce_max=fn`` (each sums / maxes its tensor in place over the ranks; both or neither): the
    forward exchanges B floats (MAX of ``m``, giving M) and one (2, B) float64 tensor (SUM of ``[s exp(m - M), lin]``),
    then ``lse = M + log S``, ``rows = w lse + lin``, ``loss = rows.sum() / B``: complete and equal on every rank.  The
    backward is ``grad_part`` with that lse; it sums dv (B x c floats) over the ranks before the stage-1 backward, so
    core / R / S receive their complete gradients, identical on every rank -- do not average them again;
    ``O_loc.grad`` is local.  A block without rows contributes ``m = -inf, s = 0, lin = 0``, zero dv and an empty gO
    and still calls both functions.

    ``lse=`` (float64 (B,), the GLOBAL log-sum-exp, e.g. ``ce_merge_lse`` of every block's ``ce_partials_block_1vN``;
    anything else raises): no exchange.  This is how ONE GPU emulates P ranks, block after block.  The result is the
    block's SHARE ``(1 / B) sum_d (w_d lse_d sigma_d + lin_d)`` with ``sigma_d = s_d exp(m_d - lse_d)`` the block's
    softmax mass; over a partition of [0, n_ent) the sigmas sum to 1 and the shares to the loss.  Its backward is
    ``grad_part`` with this lse (cast to float32 only at the kernel call): the block's share of the gradients of core,
    R and S, and the gradient of ``O_loc`` -- summed / concatenated over the partition, the gradients of the loss.
    (``lse`` is data here, not a function of the block: the share is differentiated as part of the whole loss.)

    Neither: only for the whole range (``col0 == 0``, ``n_local == n_ent``); a proper block raises ``ValueError``,
    because its own log-sum-exp is not the loss.  ``lse`` with a collective, or one collective without the other,
    raises ``ValueError`` too.

    float32, ``c <= 208``, ``c % 4 == 0`` (anything else raises; no fallback); ``max_pos`` and the ``index_check``
    policy as ``ce_loss_1vN(matrix_free=True)``; ``max_pos`` bounds the CSR entries of the batch's queries in all
    blocks.  Under ``no_grad`` only the forward sweep runs.  ``B == 0``: a zero loss and zero gradients."""
    # (the mode is checked first: a wrong combination is named before anything touches a device)
    return _ce_block_loss(_HipCeBlockLoss, core, R, S, O_loc, col0, n_ent, subject_idx, relation_idx, flt, item_ids,
                          label_smoothing, max_pos, all_reduce, all_reduce_max, lse)


def score_1vN(core, R, S, O, subject_idx, relation_idx, sigmoid=True, exact=False, sigmoid_mode=None,
              out_dtype=torch.float32, tables=None):
    """``sigmoid((G x_0 R[r] x_1 S[h]) . O^T)`` for a batch of (h, r) queries -> ``(B, N)``.

    Same operands and result as the body of the reference's ``score_fn``
    (asymmetric/R_TuckER.py:43-48; symmetric: pass ``S is O``).  ``exact=True``
    selects the exact-fp32 MFMA score kernel instead of the split-fp16 one;
    ``sigmoid_mode`` ("fast" | "exact") picks the logistic of the fused epilogue.
    ``out_dtype=torch.bfloat16`` (bf16 operands, no autograd): the scores are rounded to bf16 in the
    kernel -- the dtype the reference's bf16 model returns -- which halves the dominant HBM traffic;
    bit-identical to ``score_1vN(...).to(torch.bfloat16)``.
    ``tables`` (no autograd): the prebuilt relation tables of these parameters (``relation_tables(core, R)``);
    stage 1 then only does the subject-mode contraction -- same bits as without them.
    """
    if _wants_grad(core, R, S, O):
        if out_dtype != torch.float32:
            raise RuntimeError("bfloat16 scores are an inference option (no autograd)")
        return _Score1vN.apply(core, R, S, O, subject_idx, relation_idx, sigmoid, exact, sigmoid_mode)
    return _forward(core, R, S, O, subject_idx, relation_idx, sigmoid, exact, want_v=False, sigmoid_mode=sigmoid_mode,
                    out_dtype=out_dtype, tables=tables)[0]


def score_1vN_into(core, R, S, O, subject_idx, relation_idx, out, sigmoid=True, exact=False, sigmoid_mode=None,
                   tables=None):
    """``score_1vN`` writing into a caller-provided (B, N) buffer (row stride >= N; float32, or bfloat16
    for bf16 operands with the fast logistic); no autograd.  Used by the entity-sharded scorer so the
    local block lands in its all-gather slot."""
    with torch.no_grad():
        _forward(core, R, S, O, subject_idx, relation_idx, sigmoid, exact, want_v=False,
                 sigmoid_mode=sigmoid_mode, out=out, out_dtype=out.dtype, tables=tables)
    return out


def query_vectors_part(core, R, S, subject_idx, relation_idx, tables, part, n_parts, out):
    """Stage 1 for the queries whose relation id is congruent to ``part`` modulo ``n_parts`` only, against the prebuilt
    relation ``tables``: their rows of ``out`` (B, c) fp32 are written, the others left untouched
    (``rtk_query_vectors_from_tables_part_*``; the entity-sharded scorer's ``stage1="relation"``)."""
    op = _Operands(core, R, S, None, subject_idx, relation_idx)
    B, c, dev = op.B, op.c, op.dev
    if tuple(out.shape) != (B, c) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"out must be a contiguous float32 ({B}, {c}) tensor on {dev}")
    op.check_tables(tables)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        ws = op.workspace(sp, tables)
        _lib.check(_entry("rtk_query_vectors_from_tables_part", op.bf16)(
            tables.data_ptr(), op.R.shape[0], op.b, c, op.S.data_ptr(), op.S.shape[0], op.r.data_ptr(), op.h.data_ptr(), B,
            int(part), int(n_parts), out.data_ptr(), ws.data_ptr(), ws.numel(), sp), "rtk_query_vectors_from_tables_part")
        _strict_check(ws, sp)
    return out


def query_vectors(core, R, S, subject_idx, relation_idx, tables=None, packed=False):
    """Stage 1 only: ``v[d] = S[h_d] . (G x_0 R[r_d])`` -> ``(B, c)`` fp32 (R_TuckER.py:43-46).
    ``packed=True`` returns ``(v, q_packed)`` with the packed query planes the score kernels consume."""
    op = _Operands(core, R, S, None, subject_idx, relation_idx)
    B, c, dev = op.B, op.c, op.dev
    v = torch.empty((B, c), dtype=torch.float32, device=dev)
    qp = torch.empty(_size("rtk_packed_query_bytes", op.dcode, B, c), dtype=torch.uint8, device=dev) if packed else None
    if B > 0:
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            _strict_check(_stage1(op, sp, tables, v, qp), sp)
    return (v, qp) if packed else v


def pack_query_vectors(v, dtype):
    """Packed query planes (csrc/rtk_pack.h) of fp32 query vectors ``v (B, c)`` for the score kernels of
    operand type ``dtype`` -- the hand-over when stage 1 ran elsewhere (entity-sharded scoring with
    stage 1 split over the ranks: every rank contracts its slice of the batch, the B x c vectors are
    all-gathered, each rank packs them and scores its entity shard)."""
    _require_gpu("v", v)
    v = v.contiguous().float()
    B, c = v.shape
    dcode = _dtype_code(dtype == torch.bfloat16)
    qp = torch.empty(_size("rtk_packed_query_bytes", dcode, B, c), dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(_lib.load().rtk_pack_query_vectors(v.data_ptr(), B, c, dcode, qp.data_ptr(), _stream_ptr(v.device)),
                   "rtk_pack_query_vectors")
    return qp


def score_packed_into(qp, B, O, out, sigmoid=True, sigmoid_mode=None):
    """Stage 2 alone: ``out[d, j] = logistic(v_d . O[j])`` from packed query planes into a (B, n_local)
    buffer (float32, or bfloat16 for bf16 operands)."""
    _require_gpu("O", O)
    dev = O.device
    bf16 = O.dtype == torch.bfloat16
    O = O.contiguous()
    N = O.shape[0]
    flags = _score_flags(sigmoid, sigmoid_mode, out.dtype, bf16)
    if tuple(out.shape) != (B, N) or out.stride(1) != 1 or out.device != dev:
        raise RuntimeError(f"out must be ({B}, {N}) on {dev} with unit column stride")
    with torch.cuda.device(dev):
        _stage2(bf16, _stream_ptr(dev), None, qp, O, out, flags)
    return out


_topk_scores = {}   # (device index, stream, dtype) -> score buffer of topk_1vN, reused by every call on that stream


def _topk_score_buffer(device, stream_ptr, B, N, dtype):
    """(B, N) view, rows on 128-byte boundaries, of the per-stream buffer topk_1vN scores into: its scores are consumed
    by the select on the same stream before the next call overwrites them."""
    key = (device.index, stream_ptr, dtype)
    pitch = _row_pitch(N, dtype)
    buf = _topk_scores.get(key)
    if buf is None or buf.numel() < B * pitch:
        buf = _topk_scores[key] = torch.empty(max(B * pitch, 1), dtype=dtype, device=device)
    return buf[:B * pitch].view(B, pitch)[:, :N]


@torch.no_grad()
def topk_1vN(core, R, S, O, subject_idx, relation_idx, k, flt=None, keep_idx=None, sigmoid=True, sigmoid_mode=None,
             score_dtype=torch.float32, tables=None, entity_block=None, matrix_free=False):
    """Filtered top-k link prediction: the ``k`` most likely objects of every ``(h, r, ?)`` query, best first, as
    ``(values (B, k) float32, ids (B, k) int64)`` -- the filtered, stable descending sort of ``score_1vN``'s rows cut
    at k, without sorting them (``evaluation.filtered_topk``).  ``flt`` (a ``DeviceFilter``): the known-true objects
    of each query's pair (``flt.slots_of``) are left out, except ``keep_idx[d]``.  Rows with fewer than k candidates
    are padded with (-inf, -1).  Inference only (no autograd).

    Default: stage 1 once, stage 2 into a per-stream buffer reused across calls, then the select; the scores are
    bit-identical to ``score_1vN`` with the same arguments (``score_dtype``: its ``out_dtype``), so the result is exactly
    the filtered stable sort of ``score_1vN``'s output.
    ``entity_block=n``: the entities are scored ``n`` at a time into a (B, n) buffer (``score_packed_into`` on the packed
    query vectors), each block's top k is selected and merged into the running top k -- memory B x n instead of B x N.
    Block scores may differ from full-width scores in the last bits (the fp32 kernel's fifth column group depends on
    the column count, ``cg_fifth_group_columns``); the result is exact for the scores as computed.
    ``matrix_free=True``: no scores are stored at all (``topk_block_1vN`` on the whole range; ``rtk_score_topk_*``) --
    memory B x N / 128 floats plus B x 128 k candidates, the queries taken in chunks that keep the workspace under
    ``TOPK_STREAM_WS_BYTES``.  The result is exactly ``filtered_topk`` on the probabilities of the fp32 ws score kernel
    (bf16 operands: the bf16 kernel's), the contract of ``rank_1vN``, and the same for every partition into blocks.
    Probabilities only (``sigmoid=True``), float32 scores, ``k <= 128``, fp32 ``c <= 208`` with ``c % 4 == 0``, bf16
    ``c <= 512``; not together with ``entity_block``.  Anything else raises: there is no fallback."""
    from .evaluation import filtered_topk
    k = int(k)
    if matrix_free:
        if entity_block is not None:
            raise ValueError("matrix_free=True stores no scores: entity_block does not apply (pass one of the two)")
        if score_dtype != torch.float32:
            raise ValueError(f"matrix_free=True selects on float32 probabilities, got score_dtype = {score_dtype}")
        if not sigmoid:
            raise ValueError("matrix_free=True is taken on probabilities: sigmoid=True (raw logits are not covered)")
        _check_topk_stream_k(k)
        op = _Operands(core, R, S, O, subject_idx, relation_idx)
        B, dev = op.B, op.dev
        slots = flt.slots_of(op.h, op.r) if flt is not None else None
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            qp = _packed_buffer(dev, sp, _size("rtk_packed_query_bytes", op.dcode, B, op.c))
            if B > 0:
                _strict_check(_stage1(op, sp, tables, None, qp), sp)
        return topk_block_1vN(qp, B, op.O, 0, op.O.shape[0], k, flt=flt, slots=slots, keep_idx=keep_idx,
                              sigmoid_mode=sigmoid_mode)
    if not 1 <= k <= 1024:
        raise ValueError(f"k = {k}: the selection takes 1 <= k <= 1024")
    op = _Operands(core, R, S, O, subject_idx, relation_idx)
    B, N, dev = op.B, op.O.shape[0], op.dev
    slots = flt.slots_of(op.h, op.r) if flt is not None else None
    if entity_block is None:
        with torch.cuda.device(dev):
            out = _topk_score_buffer(dev, _stream_ptr(dev), B, N, score_dtype)
        _forward(core, R, S, O, op.h, op.r, sigmoid, False, want_v=False, sigmoid_mode=sigmoid_mode, out=out,
                 out_dtype=score_dtype, tables=tables)
        return filtered_topk(out, k, flt, keep_idx=keep_idx, slots=slots)
    n = int(entity_block)
    if n <= 0:
        raise ValueError(f"entity_block must be positive, got {entity_block}")
    if not _packed_stage2(op.c, exact=False):
        raise RuntimeError(f"entity_block needs the packed score kernels (object rank c <= {_PACKED_MAX_C})")
    _score_flags(sigmoid, sigmoid_mode, score_dtype, op.bf16)          # (the score buffer's dtype is valid)
    _, qp = query_vectors(core, R, S, op.h, op.r, tables=tables, packed=True)
    with torch.cuda.device(dev):
        buf = _topk_score_buffer(dev, _stream_ptr(dev), B, min(n, max(N, 1)), score_dtype)
    values = torch.full((B, k), float("-inf"), dtype=torch.float32, device=dev)
    ids = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    for lo in range(0, N, n):
        nb = min(n, N - lo)
        blk = buf[:, :nb]
        score_packed_into(qp, B, op.O[lo:lo + nb], blk, sigmoid=sigmoid, sigmoid_mode=sigmoid_mode)
        bv, bi = filtered_topk(blk, k, flt, keep_idx=keep_idx, slots=slots, col0=lo)
        # running list first: its ids are all below lo, so tied values stay in ascending id order
        values, ids = (bv, bi) if lo == 0 else filtered_topk(torch.cat([values, bv], 1), k, ids=torch.cat([ids, bi], 1))
    return values, ids


def _rank_operands(core, R, S, O, subject_idx, relation_idx, object_idx, flt):
    """``(op, t, slots)`` of a ranking call on the whole entity range: the checked operands, the queries' object ids and
    their filter slots (None without ``flt`` or without queries)."""
    nt, nh = torch.as_tensor(object_idx).numel(), torch.as_tensor(subject_idx).numel()
    if nt != nh:
        raise RuntimeError(f"object_idx has {nt} entries for {nh} queries")
    op = _Operands(core, R, S, O, subject_idx, relation_idx)
    t = _idx("object_idx", object_idx, op.dev)
    return op, t, flt.slots_of(op.h, op.r) if flt is not None and op.B else None


def _packed_queries(op, sp, tables):
    """Stage 1 of ``op``'s queries on stream ``sp`` into the device's packed-plane buffer."""
    qp = _packed_buffer(op.dev, sp, _size("rtk_packed_query_bytes", op.dcode, op.B, op.c))
    _stage1(op, sp, tables, None, qp)
    return qp


@torch.no_grad()
def rank_1vN(core, R, S, O, subject_idx, relation_idx, object_idx, flt=None, want_bce=False, sigmoid_mode=None,
             tables=None, rank_type="stable"):
    """Filtered rank of each ``(h, r, t)`` query against every entity -> int32 ``(B,)``, or ``(ranks, bce_rows float64)``
    with ``want_bce`` -- what ``evaluation.filtered_ranks`` gives on ``score_1vN``'s probabilities, without forming the
    (B, N) score matrix (``rtk_score_rank_*``: the kernels of ``rank_targets_block`` and ``rank_counts_block_1vN`` on the
    whole range as one block -- target scores, an entity-stationary pass that scores and counts, the filter correction, a
    finish pass; no score is stored).  ``flt`` (a
    ``DeviceFilter``): the other known-true objects of each query's pair count as probability 0.  Ranks are those of
    ``filtered_ranks`` over the fp32 ws score kernel's output (bf16 operands: the bf16 kernel's); the default fp32
    kernel differs from it only on ``cg_fifth_group_columns``.  Inference only.  An ``object_idx`` outside [0, N)
    raises ``IndexError`` by the ``index_check`` policy.

    ``rank_type``: "stable" (the default) is the rank above, the position in a stable descending sort.  "optimistic",
    "realistic" and "pessimistic" give float64 ranks from the tie counts instead (``rank_ties_1vN``,
    ``ranks_from_tie_counts``); they do not go with ``want_bce``."""
    _check_rank_type(rank_type)
    if rank_type != "stable":
        if want_bce:
            raise ValueError(f"want_bce goes with rank_type='stable' only, not {rank_type!r}")
        greater, equal = rank_ties_1vN(core, R, S, O, subject_idx, relation_idx, object_idx, flt=flt,
                                       sigmoid_mode=sigmoid_mode, tables=tables)
        return ranks_from_tie_counts(greater, equal, rank_type)
    op, t, slots = _rank_operands(core, R, S, O, subject_idx, relation_idx, object_idx, flt)
    B, N, dev = op.B, op.O.shape[0], op.dev
    flags = _score_flags(True, sigmoid_mode, torch.float32, op.bf16)
    ranks = torch.empty(B, dtype=torch.int32, device=dev)
    bce = torch.empty(B, dtype=torch.float64, device=dev) if want_bce else None
    if B == 0:
        return (ranks, bce) if want_bce else ranks
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        qp = _packed_queries(op, sp, tables)
        ws = _workspace(dev, sp, _size("rtk_score_rank_workspace_bytes", op.dcode, B, N, op.c))
        _lib.check(_entry("rtk_score_rank", op.bf16)(
            qp.data_ptr(), B, op.c, op.O.data_ptr(), N, t.data_ptr(),
            slots.data_ptr() if slots is not None else None,
            flt.pair_ptr.data_ptr() if slots is not None else None,
            flt.pair_obj.data_ptr() if slots is not None else None,
            flags, ranks.data_ptr(), bce.data_ptr() if want_bce else None, ws.data_ptr(), ws.numel(), sp),
            "rtk_score_rank")
        _strict_check(ws, sp)
    return (ranks, bce) if want_bce else ranks


class _Block:
    """The checked operands of a ranking step on one entity block: packed query planes of ``B`` queries, the block's
    rows ``O_loc`` of the (n_ent, c) entity matrix starting at global row ``col0``, the queries' object ids."""
    __slots__ = ("qp", "B", "O", "n_loc", "c", "col0", "n_ent", "t", "dev", "bf16", "dcode")

    def __init__(self, qp, B, O_loc, col0, n_ent, object_idx):
        _require_gpu("O_loc", O_loc)
        _require_gpu("q_packed", qp)
        if O_loc.dtype not in (torch.float32, torch.bfloat16) or O_loc.dim() != 2:
            raise RuntimeError(f"O_loc must be a float32 or bfloat16 (n_local, c) matrix, got {O_loc.dtype} "
                               f"{tuple(O_loc.shape)}")
        self.dev = dev = O_loc.device
        self.bf16 = O_loc.dtype == torch.bfloat16
        self.dcode = _dtype_code(self.bf16)
        self.O = O_loc.contiguous()
        self.n_loc, self.c = self.O.shape
        self.B, self.col0, self.n_ent = int(B), int(col0), int(n_ent)
        if self.B < 0:
            raise RuntimeError(f"B = {B} must be >= 0")
        need = _size("rtk_packed_query_bytes", self.dcode, self.B, self.c)
        if qp.dtype != torch.uint8 or qp.device != dev or not qp.is_contiguous() or qp.numel() < need:
            raise RuntimeError(f"q_packed must be a contiguous uint8 tensor of >= {need} bytes on {dev} "
                               "(query_vectors(..., packed=True) / pack_query_vectors)")
        self.qp = qp
        if self.col0 < 0 or self.n_loc < 1 or self.col0 + self.n_loc > self.n_ent:
            raise RuntimeError(f"block [{self.col0}, {self.col0} + {self.n_loc}) is not a non-empty part of "
                               f"[0, n_ent = {self.n_ent})")
        self.t = None                                     # (the top-k step has no queried objects)
        if object_idx is not None:
            nt = torch.as_tensor(object_idx).numel()
            if nt != self.B:
                raise RuntimeError(f"object_idx has {nt} entries for {self.B} queries")
            self.t = _idx("object_idx", object_idx, dev)

    def workspace(self, sp):
        return _workspace(self.dev, sp, _size("rtk_score_rank_part_workspace_bytes", self.dcode, self.B, self.n_loc, self.c))


@torch.no_grad()
def rank_targets_block(qp, B, O_loc, col0, n_ent, object_idx, sigmoid_mode=None):
    """Step 1 of the matrix-free ranking on an entity block (``rtk_score_rank_targets_*``): ``pt[d]`` = probability of
    ``(query d, object_idx[d])`` where ``col0 <= object_idx[d] < col0 + n_local``, ``-inf`` elsewhere -> float32 ``(B,)``.
    ``qp``: packed query planes (``query_vectors(..., packed=True)`` / ``pack_query_vectors``); ``O_loc``: rows
    ``[col0, col0 + n_local)`` of the (n_ent, c) entity matrix; ``object_idx``: GLOBAL ids.  The maximum over the
    blocks completes ``pt``.  An id outside [0, n_ent) raises ``IndexError`` by the ``index_check`` policy."""
    b = _Block(qp, B, O_loc, col0, n_ent, object_idx)
    flags = _score_flags(True, sigmoid_mode, torch.float32, b.bf16)
    pt = torch.empty(b.B, dtype=torch.float32, device=b.dev)
    if b.B == 0:
        return pt
    with torch.cuda.device(b.dev):
        sp = _stream_ptr(b.dev)
        ws = b.workspace(sp)
        _lib.check(_entry("rtk_score_rank_targets", b.bf16)(
            b.qp.data_ptr(), b.B, b.c, b.O.data_ptr(), b.n_loc, b.col0, b.n_ent, b.t.data_ptr(), flags, pt.data_ptr(),
            ws.data_ptr(), ws.numel(), sp), "rtk_score_rank_targets")
        _strict_check(ws, sp)
    return pt


def _block_filter(b, flt, slots, keep_idx=None):
    """``(slots, keep_idx)`` of a block call as int64 index tensors on the block's device, one entry per query (None
    stays None); ``slots`` go with ``flt``, the ``DeviceFilter`` that holds the CSR."""
    if flt is not None:
        if slots is None:
            raise ValueError("filtering needs the queries' filter slots: slots=flt.slots_of(subject_idx, relation_idx)")
        slots = _idx("slots", slots, b.dev)
        if slots.numel() != b.B:
            raise RuntimeError(f"slots has {slots.numel()} entries for {b.B} queries")
    elif slots is not None:
        raise ValueError("slots need flt (the DeviceFilter that holds the CSR)")
    if keep_idx is not None:
        keep_idx = _idx("keep_idx", keep_idx, b.dev)
        if keep_idx.numel() != b.B:
            raise RuntimeError(f"keep_idx has {keep_idx.numel()} entries for {b.B} queries")
    return slots, keep_idx


def _count_step(name, ws_bytes, b, pt, flt, slots, sigmoid_mode, out0, out1):
    """A counting step on block ``b``: the entry ``name`` (``_f32`` / ``_bf16``; workspace of ``ws_bytes``) on the
    completed target scores ``pt`` and the filter's CSR (NULLs without ``flt``) into ``out0``, ``out1`` (None: NULL)."""
    flags = _score_flags(True, sigmoid_mode, torch.float32, b.bf16)
    if (not isinstance(pt, torch.Tensor) or pt.dtype != torch.float32 or pt.device != b.dev or pt.numel() != b.B):
        raise RuntimeError(f"pt must be a float32 tensor of {b.B} target scores on {b.dev}")
    pt = pt.contiguous().view(-1)
    slots, _ = _block_filter(b, flt, slots)
    csr = (None,) * 3 if flt is None else (slots.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    if b.B == 0:
        return
    with torch.cuda.device(b.dev):
        sp = _stream_ptr(b.dev)
        ws = _workspace(b.dev, sp, _size(ws_bytes, b.dcode, b.B, b.n_loc, b.c))
        _lib.check(_entry(name, b.bf16)(
            b.qp.data_ptr(), b.B, b.c, b.O.data_ptr(), b.n_loc, b.col0, b.n_ent, pt.data_ptr(), b.t.data_ptr(), *csr, flags,
            out0.data_ptr(), None if out1 is None else out1.data_ptr(), ws.data_ptr(), ws.numel(), sp), name)


@torch.no_grad()
def rank_counts_block_1vN(qp, B, O_loc, col0, n_ent, pt, object_idx, flt=None, slots=None, want_bce=False,
                          sigmoid_mode=None):
    """Step 2 (``rtk_score_rank_counts_*``): this block's share of the rank count -> int32 ``(B,)``, or
    ``(counts, bce_rows float64)`` with ``want_bce``; nothing of size B x n_local is written.  ``pt``: the completed
    target scores (float32, B).  ``flt`` (a ``DeviceFilter``) with ``slots`` (``flt.slots_of(h, r)``): the queries'
    other known-true objects count as probability 0.  Summed over any partition of [0, n_ent) into blocks,
    ``1 + counts`` equals ``rank_1vN``'s ranks exactly."""
    b = _Block(qp, B, O_loc, col0, n_ent, object_idx)
    counts = torch.empty(b.B, dtype=torch.int32, device=b.dev)
    bce = torch.empty(b.B, dtype=torch.float64, device=b.dev) if want_bce else None
    _count_step("rtk_score_rank_counts", "rtk_score_rank_part_workspace_bytes", b, pt, flt, slots, sigmoid_mode, counts, bce)
    return (counts, bce) if want_bce else counts


RANK_TYPES = ("stable", "optimistic", "realistic", "pessimistic")


def _check_rank_type(rank_type):
    if rank_type not in RANK_TYPES:
        raise ValueError(f"rank_type = {rank_type!r}: one of 'stable', 'optimistic', 'realistic', 'pessimistic'")


def ranks_from_tie_counts(greater, equal, rank_type):
    """The rank of the given type from the two tie counts -> float64: optimistic ``1 + greater``, pessimistic
    ``1 + greater + equal``, realistic their mean ``1 + greater + equal / 2``.  (The stable rank needs the ids of the
    tied competitors, not only their number: ``rank_1vN`` returns it.)"""
    if rank_type == "stable" or rank_type not in RANK_TYPES:
        raise ValueError(f"rank_type = {rank_type!r}: the tie counts give 'optimistic', 'realistic' or 'pessimistic' "
                         "ranks ('stable' is rank_1vN's own)")
    g, e = torch.as_tensor(greater).to(torch.float64), torch.as_tensor(equal).to(torch.float64)
    share = {"optimistic": 0.0, "realistic": 0.5, "pessimistic": 1.0}[rank_type]
    return 1.0 + g + share * e


@torch.no_grad()
def rank_tie_counts_block_1vN(qp, B, O_loc, col0, n_ent, pt, object_idx, flt=None, slots=None, sigmoid_mode=None):
    """This block's share of the two counts every tie-aware rank derives from (``rtk_score_rank_tie_counts_*``) ->
    ``(greater, equal)``, int32 ``(B,)`` each: the entities j != t of the block with ``p'_j > pt`` and with
    ``p'_j == pt`` (IEEE comparison; a NaN never counts).  Arguments, filter rule and exactness as
    ``rank_counts_block_1vN``: summed over any partition of [0, n_ent) into blocks the counts equal the whole range's,
    and ``1 + greater <= rank_1vN <= 1 + greater + equal``."""
    b = _Block(qp, B, O_loc, col0, n_ent, object_idx)
    greater = torch.empty(b.B, dtype=torch.int32, device=b.dev)
    equal = torch.empty(b.B, dtype=torch.int32, device=b.dev)
    _count_step("rtk_score_rank_tie_counts", "rtk_score_rank_ties_workspace_bytes", b, pt, flt, slots, sigmoid_mode, greater,
                equal)
    return greater, equal


@torch.no_grad()
def rank_ties_1vN(core, R, S, O, subject_idx, relation_idx, object_idx, flt=None, sigmoid_mode=None, tables=None):
    """The tie counts of each ``(h, r, t)`` query against every entity, without the (B, N) score matrix ->
    ``(greater, equal)`` int32 ``(B,)``: the one-block call (``rank_targets_block``, then
    ``rank_tie_counts_block_1vN``, at ``col0 = 0``).  ``equal > 0`` marks a query whose rank the tie rule decides;
    ``ranks_from_tie_counts`` turns the counts into optimistic, realistic or pessimistic ranks.  Operands, filter and
    error policy as ``rank_1vN``."""
    op, t, slots = _rank_operands(core, R, S, O, subject_idx, relation_idx, object_idx, flt)
    B, N, dev = op.B, op.O.shape[0], op.dev
    if B == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        qp = _packed_queries(op, _stream_ptr(dev), tables)
        pt = rank_targets_block(qp, B, op.O, 0, N, t, sigmoid_mode=sigmoid_mode)
        return rank_tie_counts_block_1vN(qp, B, op.O, 0, N, pt, t, flt=flt, slots=slots, sigmoid_mode=sigmoid_mode)


# Workspace bound of one rtk_score_topk_* call: topk_block_1vN takes the queries in chunks (multiples of the 32-query
# packed tile) whose tile maxima and candidates fit.  Chunking by query is exact.
TOPK_STREAM_WS_BYTES = 256 << 20
TOPK_STREAM_MAX_K = 128


def _check_topk_stream_k(k):
    if not 1 <= k <= TOPK_STREAM_MAX_K:
        raise ValueError(f"k = {k}: the matrix-free top-k takes 1 <= k <= {TOPK_STREAM_MAX_K}")


def _topk_stream_chunk(dcode, B, n_loc, c, k):
    """Queries per ``rtk_score_topk_*`` call: all B when their workspace fits ``TOPK_STREAM_WS_BYTES``, else the largest
    multiple of 32 that does (at least 32)."""
    if B <= 32 or _size("rtk_score_topk_workspace_bytes", dcode, B, n_loc, c, k) <= TOPK_STREAM_WS_BYTES:
        return B
    n_tiles = -(-n_loc // 128)
    per_query = 4 * n_tiles + (4 + 8 + 128 * 12) * min(k, n_tiles)
    return max(32, (TOPK_STREAM_WS_BYTES - 6 * 256) // per_query // 32 * 32)


@torch.no_grad()
def topk_block_1vN(qp, B, O_loc, col0, n_ent, k, flt=None, slots=None, keep_idx=None, sigmoid_mode=None):
    """Filtered top k of every query among the entity block ``O_loc`` = rows ``[col0, col0 + n_local)`` of the
    (n_ent, c) entity matrix -> ``(values (B, k) float32, ids (B, k) int64)``, GLOBAL ids, best first, padded with
    (-inf, -1); nothing of size B x n_local is written (``rtk_score_topk_*``: tile maxima in an entity-stationary
    pass, their correction for the filter, the k best tiles, their candidates, the select).  The sibling of
    ``rank_counts_block_1vN``: ``qp`` are packed query planes, ``flt`` (a ``DeviceFilter``) with ``slots``
    (``flt.slots_of(h, r)``) removes each query's known-true objects except ``keep_idx[d]``.  Exactly
    ``filtered_topk(P, k, flt, slots=slots, keep_idx=keep_idx, col0=col0)`` on the block's probabilities P of the fp32
    ws score kernel (bf16 operands: the bf16 kernel's); the lists of the blocks of any partition of [0, n_ent),
    concatenated in ascending block order and merged with ``filtered_topk(values, k, ids=ids)``, equal the whole
    range's list.  Limits as ``topk_1vN(matrix_free=True)``."""
    k = int(k)
    _check_topk_stream_k(k)
    b = _Block(qp, B, O_loc, col0, n_ent, None)
    flags = _score_flags(True, sigmoid_mode, torch.float32, b.bf16)
    slots, keep_idx = _block_filter(b, flt, slots, keep_idx)
    if _size("rtk_score_topk_workspace_bytes", b.dcode, max(b.B, 1), b.n_loc, b.c, k) == 0:
        raise RuntimeError(f"topk_block_1vN: object rank c = {b.c} is not covered (float32: c <= 208 and c % 4 == 0; "
                           "bfloat16: c <= 512); there is no fallback")
    values = torch.empty((b.B, k), dtype=torch.float32, device=b.dev)
    ids = torch.empty((b.B, k), dtype=torch.int64, device=b.dev)
    if b.B == 0:
        return values, ids
    chunk = _topk_stream_chunk(b.dcode, b.B, b.n_loc, b.c, k)
    tile_bytes = _size("rtk_packed_query_bytes", b.dcode, 32, b.c)
    fn = _entry("rtk_score_topk", b.bf16)
    with torch.cuda.device(b.dev):
        sp = _stream_ptr(b.dev)
        ws = _workspace(b.dev, sp, _size("rtk_score_topk_workspace_bytes", b.dcode, min(chunk, b.B), b.n_loc, b.c, k))
        for q0 in range(0, b.B, chunk):
            nq = min(chunk, b.B - q0)
            _lib.check(fn(
                b.qp.data_ptr() + (q0 // 32) * tile_bytes, nq, b.c, b.O.data_ptr(), b.n_loc, b.col0, b.n_ent,
                slots.data_ptr() + 8 * q0 if flt is not None else None,
                flt.pair_ptr.data_ptr() if flt is not None else None,
                flt.pair_obj.data_ptr() if flt is not None else None,
                keep_idx.data_ptr() + 8 * q0 if keep_idx is not None else None,
                k, flags, values.data_ptr() + 4 * k * q0, ids.data_ptr() + 8 * k * q0, ws.data_ptr(), ws.numel(), sp),
                "rtk_score_topk")
    return values, ids


def _candidates(name, t, B, dev):
    """``(tensor, ld_cand, K)`` of a (B, K) int64 candidate matrix on ``dev`` with unit column stride; a row broadcast
    over the batch (``cand.expand(B, K)``, row stride 0) is one shared list (``ld_cand = 0``)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2:
        raise RuntimeError(f"{name} must be an int64 (B, K) tensor, got "
                           + (f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else str(type(t))))
    _require_gpu(name, t)
    if t.device != dev:
        raise RuntimeError(f"{name} is on {t.device}, the operands on {dev}")
    if t.shape[0] != B:
        raise RuntimeError(f"{name} has {t.shape[0]} rows for {B} queries")
    K = t.shape[1]
    if K > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{name} must have unit column stride")
    ld = _ld(t)
    if ld != 0 and ld < K:
        raise RuntimeError(f"{name}: row stride {ld} below K = {K} (rows must not overlap)")
    return t, ld, K


def _candidate_forward(op, cand, ld, K, flags, tables, want_v):
    """Stage 1 into fp32 query vectors, then ``rtk_score_candidates_*`` -> (B, K) fp32 scores, and v when asked."""
    B, dev = op.B, op.dev
    out = torch.empty((B, K), dtype=torch.float32, device=dev)
    if B == 0 or K == 0:
        return out, (torch.empty((B, op.c), dtype=torch.float32, device=dev) if want_v else None)
    v = torch.empty((B, op.c), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        ws = _stage1(op, sp, tables, v, None)
        _lib.check(_entry("rtk_score_candidates", op.bf16)(
            v.data_ptr(), B, op.c, op.O.data_ptr(), op.O.shape[0], cand.data_ptr(), ld, K, out.data_ptr(), K, flags,
            ws.data_ptr(), ws.numel(), sp), "rtk_score_candidates")
        _strict_check(ws, sp)
    return out, (v if want_v else None)


# The stage-1 backward has two forms.  "gemm" (rtk_query_vectors_bwd_f32) writes W = dv . G^T and the Khatri-Rao operand,
# two (B, a*b) fp32 matrices, and runs two GEMMs on them; "stream" (rtk_query_vectors_bwd_stream_*) keeps W in registers
# and needs O(B (a + b)) bytes.  The stream form is taken where the gemm form's workspace exceeds this many bytes.  The
# limit is a MEMORY policy, not a measured crossover: the two forms have not been timed against each other for it, and
# below the limit every call is the gemm form's, bit for bit.  (Tests patch it.)
_STAGE1_BWD_GEMM_BYTES = 1 << 30


def stage1_backward_route(B, a, b, c):
    """``"gemm"`` or ``"stream"``: the form of the stage-1 backward a batch of B queries at rank (a, b, c) takes --
    ``"stream"`` iff ``rtk_query_bwd_workspace_bytes(B, a, b, c) > _STAGE1_BWD_GEMM_BYTES``."""
    need = _lib.load().rtk_query_bwd_workspace_bytes(int(B), int(a), int(b), int(c))
    return "stream" if need > _STAGE1_BWD_GEMM_BYTES else "gemm"


def _stage1_backward(core, R, S, h, r, dv, needs):
    """(g_core, g_R, g_S) fp32 from the fp32 dv and core, R, S in their own dtype (float32 or bfloat16), by the route of
    ``stage1_backward_route``.  "gemm": ``rtk_query_vectors_bwd_f32`` on fp32 operands (bf16 ones are upcast first: three
    small copies).  "stream": ``rtk_query_vectors_bwd_stream_f32`` / ``_bf16`` on the operands as they are -- no copy."""
    lib = _lib.load()
    dev = dv.device
    a, b, c = core.shape
    B = dv.shape[0]
    if stage1_backward_route(B, a, b, c) == "gemm":
        core, R, S = (t.contiguous() for t in _f32(core, R, S))
        size, fn, name = lib.rtk_query_bwd_workspace_bytes, lib.rtk_query_vectors_bwd_f32, "rtk_query_vectors_bwd_f32"
    else:
        core, R, S = core.contiguous(), R.contiguous(), S.contiguous()
        bf16 = core.dtype == torch.bfloat16
        size, fn = lib.rtk_query_bwd_stream_workspace_bytes, _entry("rtk_query_vectors_bwd_stream", bf16)
        name = "rtk_query_vectors_bwd_stream" + ("_bf16" if bf16 else "_f32")
    gcore = torch.empty(core.shape, dtype=torch.float32, device=dev) if needs[0] else None
    gR = torch.empty(R.shape, dtype=torch.float32, device=dev) if needs[1] else None
    gS = torch.empty(S.shape, dtype=torch.float32, device=dev) if needs[2] else None
    with torch.cuda.device(dev):
        bws = torch.empty(size(B, a, b, c), dtype=torch.uint8, device=dev)
        _lib.check(fn(core.data_ptr(), a, b, c, R.data_ptr(), R.shape[0], S.data_ptr(), S.shape[0], r.data_ptr(),
                      h.data_ptr(), B, dv.data_ptr(),
                      gcore.data_ptr() if needs[0] else None,
                      gR.data_ptr() if needs[1] else None,
                      gS.data_ptr() if needs[2] else None,
                      bws.data_ptr(), bws.numel(), _stream_ptr(dev)), name)
    return gcore, gR, gS


class _ScoreCandidates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, core, R, S, O, subject_idx, relation_idx, candidates, sigmoid, sigmoid_mode):
        op = _Operands(core, R, S, O, subject_idx, relation_idx)
        cand, ld, K = _candidates("candidates", candidates, op.B, op.dev)
        flags = _score_flags(sigmoid, sigmoid_mode, torch.float32, op.bf16)
        out, v = _candidate_forward(op, cand, ld, K, flags, None, want_v=True)
        ctx.save_for_backward(op.core, op.R, op.S, op.O, op.h, op.r, cand, v, out)
        ctx.sigmoid, ctx.ld = sigmoid, ld
        return out

    @staticmethod
    def backward(ctx, grad_out):
        core, R, S, O, h, r, cand, v, out = ctx.saved_tensors
        needs = ctx.needs_input_grad
        B, K = out.shape
        N, c = O.shape
        dev = out.device
        if B == 0 or K == 0:
            return _zero_batch_grads(ctx)
        lib = _lib.load()
        grad_out = grad_out.contiguous().float()
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            if ctx.sigmoid:                   # dZ = dP * P * (1 - P); the NaN entries of bad ids are skipped below
                dZ = torch.empty_like(out)
                _lib.check(lib.rtk_sigmoid_grad_f32(grad_out.data_ptr(), out.data_ptr(), dZ.data_ptr(), out.numel(), sp),
                           "rtk_sigmoid_grad_f32")
            else:
                dZ = grad_out
            want_dv = needs[0] or needs[1] or needs[2]
            dv = torch.empty((B, c), dtype=torch.float32, device=dev) if want_dv else None
            gO = torch.empty((N, c), dtype=torch.float32, device=dev) if needs[3] else None
            nws = lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N) if needs[3] else 0
            ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
            # (the kernel reads O in the operands' own dtype; only the stage-1 backward computes on fp32 copies)
            _lib.check(_entry("rtk_score_candidates_bwd", O.dtype == torch.bfloat16)(
                dZ.data_ptr(), K, v.data_ptr(), B, c, O.data_ptr(), N, cand.data_ptr(), ctx.ld, K,
                dv.data_ptr() if want_dv else None, gO.data_ptr() if needs[3] else None, ws.data_ptr(), ws.numel(), sp),
                "rtk_score_candidates_bwd")
        g = _stage1_backward(core, R, S, h, r, dv, needs) if want_dv else (None,) * 3
        # symmetric model: S and O are the same tensor passed twice; autograd sums gS + gO
        return _grads_like(g + (gO,), core.dtype) + (None,) * 5


def score_candidates(core, R, S, O, subject_idx, relation_idx, candidates, sigmoid=True, sigmoid_mode=None,
                     tables=None):
    """``sigmoid(v_d . O[candidates[d, k]])`` -> ``(B, K)`` fp32: each query scored against its own list of K entities
    (``rtk_score_candidates_*``) instead of all N.  ``candidates``: int64 (B, K) on the operands' device, unit column
    stride; ``cand.expand(B, K)`` of one row is a list shared by every query.  A score depends only on the query, the
    entity and c: the same triple has the same bits in every list, at every K and batch split.  Differentiable with
    respect to core, R, S and O (bf16 operands: gradients computed in fp32, returned in bf16).  ``tables`` (no
    autograd): prebuilt relation tables, as for ``score_1vN``.  An id outside [0, N) gives a NaN entry and raises
    ``IndexError`` by the ``index_check`` policy."""
    if _wants_grad(core, R, S, O):
        return _ScoreCandidates.apply(core, R, S, O, subject_idx, relation_idx, candidates, sigmoid, sigmoid_mode)
    op = _Operands(core, R, S, O, subject_idx, relation_idx)
    cand, ld, K = _candidates("candidates", candidates, op.B, op.dev)
    flags = _score_flags(sigmoid, sigmoid_mode, torch.float32, op.bf16)
    return _candidate_forward(op, cand, ld, K, flags, tables, want_v=False)[0]


def score_triples(core, R, S, O, subject_idx, relation_idx, object_idx, sigmoid=True, sigmoid_mode=None, tables=None):
    """Scores of the triples ``(h, r, t)`` -> ``(B,)``: ``score_candidates`` with K = 1 (the same bits as any column
    that holds t in a candidate list of the same query)."""
    dev = core.device if isinstance(core, torch.Tensor) else None
    t = _idx("object_idx", object_idx, dev) if dev is not None and dev.type == "cuda" else object_idx
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    return score_candidates(core, R, S, O, subject_idx, relation_idx, t.reshape(-1, 1), sigmoid=sigmoid,
                            sigmoid_mode=sigmoid_mode, tables=tables).view(-1)


def _pair_stage1(op, h, t, B, sp, u, qp):
    """``rtk_pair_vectors_*``: ``u`` (B, a) fp32 and, when ``qp`` is given, its packed planes.  Returns the workspace."""
    ws = _workspace(op.dev, sp, _size("rtk_pair_vectors_workspace_bytes", op.dcode, B, op.a, op.b, op.c))
    _lib.check(_entry("rtk_pair_vectors", op.bf16)(
        op.core.data_ptr(), op.a, op.b, op.c, op.S.data_ptr(), op.S.shape[0], op.O.data_ptr(), op.O.shape[0],
        h.data_ptr(), t.data_ptr(), B, u.data_ptr(), op.a, None if qp is None else qp.data_ptr(), ws.data_ptr(), ws.numel(),
        sp), "rtk_pair_vectors")
    return ws


def _pair_queries(op, subject_idx, object_idx):
    h, t = _idx("subject_idx", subject_idx, op.dev), _idx("object_idx", object_idx, op.dev)
    if h.numel() != t.numel():
        raise RuntimeError(f"subject_idx has {h.numel()} entries, object_idx {t.numel()}")
    return h, t, h.numel()


@torch.no_grad()
def pair_vectors(core, S, O, subject_idx, object_idx, packed=False):
    """Stage 1 of relation prediction: ``u[d, i] = sum_jk G[i, j, k] S[h_d, j] O[t_d, k]`` -> ``(B, a)`` fp32
    (``rtk_pair_vectors_*``; symmetric model: pass ``S is O``).  ``packed=True`` returns ``(u, planes)`` with the packed
    planes of ``u`` (``pack_query_vectors(u, core.dtype)``'s bytes), which a score kernel takes against ``R``.  Nothing
    of size B x a*b is written.  The bits of a row depend only on ``O[t_d]``, ``S[h_d]``, the core and the dtype, not on
    the batch.  Inference only: runs under ``torch.no_grad()``, no autograd.  An id outside its table is clamped and
    raises ``IndexError`` by the ``index_check`` policy."""
    op = _Operands(core, None, S, O)
    h, t, B = _pair_queries(op, subject_idx, object_idx)
    u = torch.empty((B, op.a), dtype=torch.float32, device=op.dev)
    qp = torch.empty(_size("rtk_packed_query_bytes", op.dcode, B, op.a), dtype=torch.uint8, device=op.dev) if packed else None
    if B > 0:
        with torch.cuda.device(op.dev):
            sp = _stream_ptr(op.dev)
            _strict_check(_pair_stage1(op, h, t, B, sp, u, qp), sp)
    return (u, qp) if packed else u


@torch.no_grad()
def score_relations(core, R, S, O, subject_idx, object_idx, sigmoid=True, sigmoid_mode=None):
    """Scores of every relation for a batch of (h, ?, t) queries -> ``(B, n_rel)`` fp32: ``logistic(u_d . R[r])`` with the
    pair vectors ``u`` of ``pair_vectors``; column r is the 1-vs-all score of ``(h_d, r)`` at entity ``t_d``.  Stage 2 is
    the score kernel of the 1-vs-all path on the packed planes of ``u`` against ``R`` (bf16 operands: ``u`` is rounded to
    bf16 there, as the query vectors are); fp32 operands with a relation rank above 512 go through ``rtk_score_f32``.
    ``sigmoid_mode`` as for ``score_1vN``.  Inference only: runs under ``torch.no_grad()``, no autograd."""
    op = _Operands(core, R, S, O)
    h, t, B = _pair_queries(op, subject_idx, object_idx)
    return _relation_forward(op, h, t, B, _score_flags(sigmoid, sigmoid_mode, torch.float32, op.bf16))[0]


def _relation_forward(op, h, t, B, flags):
    """``(scores (B, n_rel) fp32, u (B, a) fp32)`` of ``score_relations``: ``rtk_pair_vectors_*``, then stage 2 on ``R``."""
    out = torch.empty((B, op.R.shape[0]), dtype=torch.float32, device=op.dev)
    u = torch.empty((B, op.a), dtype=torch.float32, device=op.dev)
    if B == 0:
        return out, u
    packed = _packed_stage2(op.a, exact=False)
    if op.bf16 and not packed:
        raise RuntimeError(f"bf16 operands: only the bf16 MFMA score kernel exists (relation rank a <= {_PACKED_MAX_C})")
    with torch.cuda.device(op.dev):
        sp = _stream_ptr(op.dev)
        qp = _packed_buffer(op.dev, sp, _size("rtk_packed_query_bytes", op.dcode, B, op.a)) if packed else None
        ws = _pair_stage1(op, h, t, B, sp, u, qp)
        _stage2(op.bf16, sp, u, qp, op.R, out, flags)
        _strict_check(ws, sp)
    return out, u


def _f32_matrix(name, t, dev=None):
    _require_gpu(name, t)
    if t.dtype != torch.float32 or t.dim() != 2 or (dev is not None and t.device != dev):
        raise RuntimeError(f"{name} must be a float32 matrix on {dev or 'the GPU'}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _pair_rows(core, X, x_idx, w, sp):
    """``rtk_pair_rows_f32`` on the stream ``sp`` -> ``(rows (B, b) fp32, workspace)``."""
    a, b, c = core.shape
    B = w.shape[0]
    rows = torch.empty((B, b), dtype=torch.float32, device=core.device)
    ws = _workspace(core.device, sp, max(256, _size("rtk_pair_rows_workspace_bytes", B, a, b, c)))
    _lib.check(_lib.load().rtk_pair_rows_f32(core.data_ptr(), a, b, c, X.data_ptr(), X.shape[0], x_idx.data_ptr(),
                                             w.data_ptr(), _ld(w), B, rows.data_ptr(), b, ws.data_ptr(), ws.numel(), sp),
               "rtk_pair_rows_f32")
    return rows, ws


@torch.no_grad()
def pair_rows(core, X, x_idx, w):
    """``rows[d, j] = sum_i w[d, i] * sum_k core[i, j, k] X[x_idx[d], k]`` -> ``(B, b)`` fp32 (``rtk_pair_rows_f32``): the
    row gradients of relation prediction.  ``core`` (a, b, c), ``X`` (n, c) and ``w`` (B, a) are float32; ``c <= 208``,
    ``c % 4 == 0``.  Nothing of size B x a*b is written; the bits of a row depend only on ``X[x_idx[d]]``, ``w[d]`` and
    the core.  An id outside [0, n) is clamped and raises ``IndexError`` by the ``index_check`` policy."""
    _require_gpu("core", core)
    if core.dtype != torch.float32 or core.dim() != 3:
        raise RuntimeError(f"core must be a float32 (a, b, c) tensor, got {core.dtype} {tuple(core.shape)}")
    core, dev = core.contiguous(), core.device
    X, w = _f32_matrix("X", X, dev).contiguous(), _f32_matrix("w", w, dev)
    idx = _idx("x_idx", x_idx, dev)
    if X.shape[1] != core.shape[2] or w.shape[1] != core.shape[0] or idx.numel() != w.shape[0]:
        raise RuntimeError(f"X {tuple(X.shape)}, w {tuple(w.shape)} and x_idx ({idx.numel()},) do not match core "
                           f"{tuple(core.shape)}")
    with torch.cuda.device(dev):
        sp = _stream_ptr(dev)
        rows, ws = _pair_rows(core, X, idx, w, sp)
        if w.shape[0] > 0:
            _strict_check(ws, sp)
    return rows


@torch.no_grad()
def core_outer(x, y, z):
    """``gG[i, j, k] = sum_d (x[d, i] * y[d, j]) * z[d, k]`` -> ``(a, b, c)`` fp32 (``rtk_core_outer_f32``): the exact fp32
    MFMA GEMM on the Khatri-Rao product of ``x`` (B, a) and ``y`` (B, b), which is never written to memory, against ``z``
    (B, c).  One chain over d ascending per element: the bits of ``rtk_gemm_f32`` on the materialised product."""
    x = _f32_matrix("x", x)
    y, z = _f32_matrix("y", y, x.device), _f32_matrix("z", z, x.device)
    if not x.shape[0] == y.shape[0] == z.shape[0]:
        raise RuntimeError(f"x {tuple(x.shape)}, y {tuple(y.shape)}, z {tuple(z.shape)} must have one row per query")
    a, b, c = x.shape[1], y.shape[1], z.shape[1]
    gG = torch.empty((a, b, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().rtk_core_outer_f32(x.data_ptr(), _ld(x), a, y.data_ptr(), _ld(y), b, z.data_ptr(), _ld(z), c,
                                                  x.shape[0], gG.data_ptr(), _stream_ptr(x.device)), "rtk_core_outer_f32")
    return gG


@torch.no_grad()
def scatter_rows(idx, rows, n_out):
    """``out[e, :] = sum_{d: idx[d] = e} rows[d, :]`` -> ``(n_out, n)`` fp32 (``rtk_scatter_rows_f32``): the ordered
    scatter, no float atomics, the same bits on every run; ids outside [0, n_out) add nothing.  ``n <= 1024``."""
    rows = _f32_matrix("rows", rows)
    dev = rows.device
    idx = _idx("idx", idx, dev)
    B, n = rows.shape
    if idx.numel() != B:
        raise RuntimeError(f"idx has {idx.numel()} entries for {B} rows")
    out = torch.empty((n_out, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(max(256, _size("rtk_scatter_rows_workspace_bytes", B)), dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().rtk_scatter_rows_f32(idx.data_ptr(), rows.data_ptr(), _ld(rows), B, n, n_out, out.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "rtk_scatter_rows_f32")
    return out


class _RelationLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, core, R, S, O, subject_idx, object_idx):
        op = _Operands(core, R, S, O)
        h, t, B = _pair_queries(op, subject_idx, object_idx)
        out, u = _relation_forward(op, h, t, B, _score_flags(False, None, torch.float32, op.bf16))
        ctx.save_for_backward(op.core, op.R, op.S, op.O, h, t, u)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        core, R, S, O, h, t, u = ctx.saved_tensors
        needs = ctx.needs_input_grad[:4]
        pdt = core.dtype                      # bf16 operands: gradients computed in fp32, returned in bf16
        B, dev = u.shape[0], u.device
        if B == 0:
            return _zero_batch_grads(ctx)
        core, R, S, O = _f32(core, R, S, O)
        lib = _lib.load()
        a, n_rel = core.shape[0], R.shape[0]
        dZ = grad_out.contiguous().float()
        g = [None] * 4
        with torch.cuda.device(dev):
            sp = _stream_ptr(dev)
            if needs[1]:                      # gR[r, i] = sum_d dZ[d, r] u[d, i]
                g[1] = torch.empty((n_rel, a), dtype=torch.float32, device=dev)
                _lib.check(lib.rtk_gemm_f32(dZ.data_ptr(), 0, n_rel, u.data_ptr(), 0, a, g[1].data_ptr(), a, n_rel, a, B, 0,
                                            sp), "rtk_gemm_f32 (gR)")
            if needs[0] or needs[2] or needs[3]:
                du = torch.empty((B, a), dtype=torch.float32, device=dev)      # du[d, i] = sum_r dZ[d, r] R[r, i]
                _lib.check(lib.rtk_gemm_f32(dZ.data_ptr(), 1, n_rel, R.data_ptr(), 0, a, du.data_ptr(), a, B, a, n_rel, 0,
                                            sp), "rtk_gemm_f32 (du)")
            if needs[2]:
                g[2] = scatter_rows(h, _pair_rows(core, O, t, du, sp)[0], S.shape[0])
            if needs[3]:
                g[3] = scatter_rows(t, _pair_rows(core.transpose(1, 2).contiguous(), S, h, du, sp)[0], O.shape[0])
            if needs[0]:                      # (ids outside their table were reported by the forward; here they are clamped)
                g[0] = core_outer(du, S.index_select(0, h.clamp(0, S.shape[0] - 1)),
                                  O.index_select(0, t.clamp(0, O.shape[0] - 1)))
        # symmetric model: S and O are the same tensor passed twice; autograd sums gS + gO
        return _grads_like(g, pdt) + (None, None)


def relation_logits(core, R, S, O, subject_idx, object_idx):
    """Logits of every relation for a batch of (h, ?, t) queries -> ``(B, n_rel)`` fp32, with gradients in core, R, S and
    O: the forward is ``score_relations(..., sigmoid=False)`` (the same bits).  The backward writes nothing of size
    B x a*b: ``du = dZ . R`` and ``gR = dZ^T . u`` by ``rtk_gemm_f32``, the row gradients of ``S[h]`` and ``O[t]`` by
    ``rtk_pair_rows_f32`` and the ordered ``rtk_scatter_rows_f32``, the core's by ``rtk_core_outer_f32``; only what
    ``requires_grad`` asks for is computed, and two runs give the same bits.  bf16 operands: the forward runs the bf16
    kernels, the backward in fp32 on the upcast operands, gradients returned in bf16.  Symmetric model: pass ``S is O``;
    autograd adds the two gradients.  Limit: the fp32 sweeps of the backward need ``b = c <= 208`` and ``c % 4 == 0``
    (anything else raises; no fallback)."""
    return _RelationLogits.apply(core, R, S, O, subject_idx, object_idx)


def relation_ce_loss(core, R, S, O, subject_idx, object_idx, relation_idx, label_smoothing=0.0):
    """Relation-classification loss: the mean softmax cross-entropy of ``relation_logits`` against ``relation_idx``
    (``F.cross_entropy`` on the small (B, n_rel) matrix).  Stands alone or as the auxiliary term next to ``bce_loss_1vN``."""
    z = relation_logits(core, R, S, O, subject_idx, object_idx)
    rel = _idx("relation_idx", relation_idx, z.device)
    if rel.numel() != z.shape[0]:
        raise RuntimeError(f"relation_idx has {rel.numel()} entries for {z.shape[0]} queries")
    return torch.nn.functional.cross_entropy(z, rel, label_smoothing=label_smoothing)


def cg_fifth_group_columns(N, c, flags=0):
    """Boolean mask (N,) of the entity columns that the default fp32 score kernel computes as FOUR K-range chains added
    in a fixed order instead of one chain -- the fifth column group of a workgroup's set in the column-group kernel
    (``rtk_score_fifth_group_columns_f32``; ``flags``: a kernel hint).  Everywhere else (all False) a score does not
    depend on how many other entities are scored with it; on these columns an entity-sharded run and a single-device
    run differ in the last bits."""
    import numpy as np
    mask = np.zeros(N, dtype=np.uint8)
    n = _lib.load().rtk_score_fifth_group_columns_f32(N, c, flags, mask.ctypes.data)
    if n < 0:
        _lib.check(n, "rtk_score_fifth_group_columns_f32")
    return mask.view(bool)


def check_device_errors(device=None):
    """Synchronise and raise ``IndexError`` if a kernel saw an out-of-range subject /
    relation id since the last check (the kernels clamp such ids instead of faulting;
    the reference raises IndexError on CPU / asserts on device).  Each workspace's word is read and
    cleared on the stream that owns it."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    bad = None
    for (di, sp), ws in list(_workspaces.items()):
        if di != dev.index:
            continue
        try:
            _check_now(ws, sp)
        except IndexError as e:
            bad = e
    if bad is not None:
        raise bad
