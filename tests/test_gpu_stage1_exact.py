"""The stage-1 forward (csrc/rtk_query.hip) through the C ABI, bit for bit against float64, and the packed query
planes byte for byte against the independent packer of tests/golden/stage1_cases.py.

Operands are integer-valued with abs-sums below 2^24 (stage1_cases.operands asserts it), so the VALU tables, the
bf16 MFMA tables, the split-fp16 GEMM tables, the fp32 GEMM with bf16 widening and both contract kernels cannot round:
rtk_relation_tables_*, rtk_query_vectors_* and rtk_query_vectors_from_tables_* must return the float64 result
exactly, whichever branch runs.  The case list reaches every label of stage1_cases.LABELS with planted relation
counts (tests/test_stage1_cases_host.py holds that equality and proves the mutants on the host).

Every call: outputs pre-filled with a sentinel (a guard past the end included), each case with v_out only, q_packed
only and both, workspaces pre-filled with 0xFF except the error word (the first 32-bit word, which the header
documents as caller-zeroed and sticky), the error word clear afterwards.  Bytes of the packed planes that no
producer may write (rows >= B of the last tile) keep the sentinel.  No invalid ids, no tolerances.
"""
import numpy as np
import pytest
import torch

import stage1_cases as sc
from exact_cases import real_values

pytestmark = pytest.mark.gpu

RTK = {"f32": 0, "bf16": 1}
GUARD = 256


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev(x, dtype="f32"):
    t = torch.from_numpy(np.ascontiguousarray(x))
    if dtype == "bf16" and t.dtype == torch.float32:
        assert torch.equal(t.bfloat16().float(), t), "operand is not a bf16 number"
        t = t.bfloat16()
    t = t.cuda()
    assert t.data_ptr() % 256 == 0
    return t


def workspace(nbytes):
    """0xFF everywhere but the caller-zeroed error word."""
    ws = torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    ws[:4] = 0
    return ws


def error_word(ws):
    return int(ws[:4].cpu().numpy().view(np.uint32)[0])


class Outputs:
    """Sentinel-filled v_out (B x c fp32) and q_packed, each with a guard behind it."""

    def __init__(self, lib, B, c, dtype, want_v, want_q):
        self.B, self.c, self.dtype = B, c, dtype
        self.v = torch.full((B * c + GUARD,), sc.SENTINEL, dtype=torch.float32, device="cuda") if want_v else None
        self.nq = int(lib.rtk_packed_query_bytes(RTK[dtype], B, c))
        self.q = torch.full((self.nq + GUARD,), sc.PACK_FILL, dtype=torch.uint8, device="cuda") if want_q else None

    def ptrs(self):
        return (self.v.data_ptr() if self.v is not None else None, self.q.data_ptr() if self.q is not None else None)

    def host(self):
        v = q = None
        if self.v is not None:
            x = self.v.cpu().numpy()
            assert np.all(x[self.B * self.c:] == sc.SENTINEL), "v_out written past row B"
            v = x[:self.B * self.c].reshape(self.B, self.c)
        if self.q is not None:
            x = self.q.cpu().numpy()
            assert np.all(x[self.nq:] == sc.PACK_FILL), "q_packed written past its end"
            q = x[:self.nq]
        return v, q


def first_difference(name, got, ref):
    bad = np.argwhere(got.astype(np.float64) != ref)
    i = tuple(bad[0])
    return f"{name}: {len(bad)} of {ref.size} elements differ; first at {i}: got {got[i]!r}, expected {ref[i]!r}"


def check(tag, dtype, v, q, v64, planes):
    """planes: pack_ref of the reference vectors for this dtype, computed once per case."""
    if v is not None:
        assert np.array_equal(v.astype(np.float64), v64), f"[{tag}] " + first_difference("v", v, v64)
    if q is not None:
        msg = sc.packed_mismatch(q, v64.astype(np.float32), dtype, ref=planes)
        assert msg is None, f"[{tag}] {msg}"


def call_full(lib, case, dtype, ops, out):
    core, R, S, rel, sub = ops
    ws = workspace(lib.rtk_workspace_bytes(RTK[dtype], case.B, case.n_rel, case.a, case.r, case.r))
    fn = lib.rtk_query_vectors_f32 if dtype == "f32" else lib.rtk_query_vectors_bf16
    rc = fn(core.data_ptr(), case.a, case.r, case.r, R.data_ptr(), case.n_rel, S.data_ptr(), case.n_sub, rel.data_ptr(),
            sub.data_ptr(), case.B, *out.ptrs(), ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert error_word(ws) == 0, "error word set by valid ids"


def call_tables(lib, case, dtype, ops):
    core, R, S, rel, sub = ops
    n = int(lib.rtk_relation_tables_bytes(case.n_rel, case.r, case.r))
    tables = torch.full((n // 4 + GUARD,), sc.SENTINEL, dtype=torch.float32, device="cuda")
    assert tables.data_ptr() % 256 == 0
    ws = workspace(lib.rtk_relation_tables_workspace_bytes(RTK[dtype], case.n_rel, case.a, case.r, case.r))
    fn = lib.rtk_relation_tables_f32 if dtype == "f32" else lib.rtk_relation_tables_bf16
    rc = fn(core.data_ptr(), case.a, case.r, case.r, R.data_ptr(), case.n_rel, tables.data_ptr(), ws.data_ptr(), ws.numel(),
            _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    return tables


def call_from_tables(lib, case, dtype, ops, tables, out, part=None):
    core, R, S, rel, sub = ops
    ws = workspace(lib.rtk_from_tables_workspace_bytes(case.B, case.n_rel))
    args = (tables.data_ptr(), case.n_rel, case.r, case.r, S.data_ptr(), case.n_sub, rel.data_ptr(), sub.data_ptr(), case.B)
    if part is None:
        fn = lib.rtk_query_vectors_from_tables_f32 if dtype == "f32" else lib.rtk_query_vectors_from_tables_bf16
        rc = fn(*args, *out.ptrs(), ws.data_ptr(), ws.numel(), _stream())
    else:
        fn = lib.rtk_query_vectors_from_tables_part_f32 if dtype == "f32" else lib.rtk_query_vectors_from_tables_part_bf16
        rc = fn(*args, part[0], part[1], out.ptrs()[0], ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert error_word(ws) == 0, "error word set by valid ids"


def output_subsets(case):
    return ((True, False), (False, True), (True, True)) if case.packed else ((True, False),)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_stage1_forward_bit_exact(lib, case):
    T64, v64 = sc.reference(case)                     # operands() asserts the 2^24 conditions
    host_ops = sc.operands(case)
    for dtype in case.dtypes:
        ops = [dev(x, dtype) for x in host_ops]
        planes = sc.pack_ref(v64.astype(np.float32), dtype) if case.packed else None
        for entry in case.entries:
            tag = f"{dtype}, {entry}: " + ", ".join(sorted(x for x in sc.route(case, dtype, entry) if "=" not in x))
            if entry == "tables":
                tables = call_tables(lib, case, dtype, ops)
                t = tables.cpu().numpy()
                assert np.all(t[T64.size:] == sc.SENTINEL), "tables written past their end"
                t = t[:T64.size].reshape(T64.shape)
                assert np.array_equal(t.astype(np.float64), T64), f"[{tag}] " + first_difference("tables", t, T64)
            for want_v, want_q in output_subsets(case):
                out = Outputs(lib, case.B, case.r, dtype, want_v, want_q)
                if entry == "full":
                    call_full(lib, case, dtype, ops, out)
                else:
                    call_from_tables(lib, case, dtype, ops, tables, out)
                check(tag, dtype, *out.host(), v64, planes)


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.parts], ids=lambda c: c.name)
def test_parts_write_their_own_rows_only(lib, case):
    T64, v64 = sc.reference(case)
    host_ops = sc.operands(case)
    rel = host_ops[3]
    for dtype in case.dtypes:
        ops = [dev(x, dtype) for x in host_ops]
        tables = call_tables(lib, case, dtype, ops)
        whole = Outputs(lib, case.B, case.r, dtype, True, False)
        call_from_tables(lib, case, dtype, ops, tables, whole)
        whole = whole.host()[0]
        for n in case.parts:
            union = np.full_like(whole, sc.SENTINEL)
            for p in range(n):
                out = Outputs(lib, case.B, case.r, dtype, True, False)
                call_from_tables(lib, case, dtype, ops, tables, out, part=(p, n))
                v = out.host()[0]
                mine = rel % n == p
                assert np.array_equal(v[mine].astype(np.float64), v64[mine]), (dtype, n, p)
                assert np.all(v[~mine] == sc.SENTINEL), f"{dtype}: part {p} of {n} wrote a foreign relation's rows"
                union[mine] = v[mine]
            assert np.array_equal(union.view(np.uint32), whole.view(np.uint32)), (dtype, n)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,c", sc.PACK_SHAPES)
def test_pack_query_vectors_on_planted_rows(lib, B, c, dtype):
    """rtk_pack_query_vectors on real-valued rows with the edge rows planted (stage1_cases.pack_rows): the pack
    arithmetic is deterministic, so the bytes equal the independent packer's."""
    v = sc.pack_rows(B, c, 1000 * B + c)
    out = Outputs(lib, B, c, dtype, False, True)
    vd = dev(v)
    rc = lib.rtk_pack_query_vectors(vd.data_ptr(), B, c, RTK[dtype], out.q.data_ptr(), _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    msg = sc.packed_mismatch(out.host()[1], v, dtype)
    assert msg is None, msg


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,B,a,r,n_rel", sc.PLANE_CASES)
def test_contract_kernels_pack_their_own_vectors(lib, name, B, a, r, n_rel, dtype):
    """Real-valued operands: the planes a contract kernel writes are the packing of the v it writes."""
    rng = np.random.default_rng(sc._seed(name))
    case = sc.Stage1Case(name, B, a, r, n_rel, n_sub=200)
    core, R, S = real_values(rng, (a, r, r)), real_values(rng, (n_rel, a)), real_values(rng, (200, r), pow2_rows=True)
    if dtype == "bf16":
        core, R, S = [torch.from_numpy(x).bfloat16().float().numpy() for x in (core, R, S)]
    rel = sc.rel_ids(((0, 9), (n_rel - 1, 1)), n_rel, B, rng)
    sub = rng.integers(0, 200, size=B).astype(np.int64)
    assert ("contract_grouped" in sc.route(case, dtype, "full")) == (B >= sc.GROUPED_MIN_B)
    ops = [dev(x, dtype) for x in (core, R, S, rel, sub)]
    out = Outputs(lib, B, r, dtype, True, True)
    call_full(lib, case, dtype, ops, out)
    v, q = out.host()
    assert np.isfinite(v).all() and np.abs(v).max() > 0
    msg = sc.packed_mismatch(q, v, dtype)
    assert msg is None, msg
