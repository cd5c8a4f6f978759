"""CPU tests of the matrix-free top-k (rtk_score_topk_*, csrc/rtk_score_topk.hip): the workspace query without a device,
and the algorithm -- tile maxima that exclude the filtered objects, the min(k, n_tiles) best tiles, their candidates in
ascending id order, the select's tie split in column order -- restated in numpy and compared with a plain stable
filtered sort.  The restatement lives here, not in the package: it pins the lemma and the tie rule, the GPU tests pin
the kernels."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 128


@pytest.fixture(scope="module")
def lib():
    from r_tucker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):   # build in-tree (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["bash", os.path.join(ROOT, "r-tucker_amd", "csrc", "build.sh")], check=True)
    return _lib.load()


def align256(x):
    return -(-x // 256) * 256


def test_workspace_bytes_without_a_device(lib):
    f = lib.rtk_score_topk_workspace_bytes
    for dtype, c in ((0, 200), (1, 512)):
        for B, N, k in ((512, 40943, 10), (8192, 1_000_000, 10), (33, 1000, 128), (1, 1, 1), (70, 129, 128)):
            T = -(-N // TILE)
            kt = min(k, T)
            want = (256 + align256(4 * B * T) + align256(4 * B * kt) + align256(8 * B * kt) + align256(512 * B * kt)
                    + align256(1024 * B * kt))
            assert f(dtype, B, N, c, k) == want
    # the only part that grows with N is the tile maxima: 1/128 of the score block
    B, k, c = 8192, 10, 200
    for N in (100_000, 125_000, 500_000):
        grow = f(0, B, 2 * N, c, k) - f(0, B, N, c, k)
        assert 0 < grow <= B * -(-N // TILE) * 4 + 256
    assert f(0, 0, 1000, 200, 10) > 0


def test_workspace_bytes_rejects_what_the_kernels_do_not_cover(lib):
    f = lib.rtk_score_topk_workspace_bytes
    assert f(0, 64, 1000, 200, 128) > 0 and f(0, 64, 1000, 200, 129) == 0 and f(0, 64, 1000, 200, 0) == 0
    assert f(0, 64, 1000, 208, 10) > 0 and f(0, 64, 1000, 212, 10) == 0       # fp32: c <= 208
    assert f(0, 64, 1000, 6, 10) == 0 and f(0, 64, 1000, 0, 10) == 0           # fp32: c % 4 == 0
    assert f(1, 64, 1000, 512, 10) > 0 and f(1, 64, 1000, 513, 10) == 0       # bf16: c <= 512
    assert f(1, 64, 1000, 7, 10) > 0
    assert f(2, 64, 1000, 8, 10) == 0 and f(0, -1, 1000, 8, 10) == 0 and f(0, 64, 0, 8, 10) == 0


def test_entry_points_validate_without_a_device(lib):
    a = 256                                         # any non-null, 256-byte-aligned address: nothing is dereferenced
    def call(fn, c, n_local, col0, n_ent, k, flags, ws_bytes=1 << 30, slot=None):
        return fn(a, 4, c, a, n_local, col0, n_ent, slot, None, None, None, k, flags, a, a, a, ws_bytes, None)
    f32, bf16 = lib.rtk_score_topk_f32, lib.rtk_score_topk_bf16
    assert call(f32, 36, 100, 0, 100, 129, 5) == -1 and b"128" in lib.rtk_last_error_string()
    assert call(f32, 36, 100, 0, 100, 0, 5) == -1
    assert call(f32, 36, 100, 0, 100, 10, 4) == -3 and b"RTK_SCORE_SIGMOID" in lib.rtk_last_error_string()
    assert call(f32, 36, 100, 0, 100, 10, 1 | 16) == -1 and b"flags" in lib.rtk_last_error_string()
    assert call(f32, 212, 100, 0, 100, 10, 5) == -3 and b"208" in lib.rtk_last_error_string()
    assert call(f32, 6, 100, 0, 100, 10, 5) == -3 and b"c % 4" in lib.rtk_last_error_string()
    assert call(bf16, 528, 100, 0, 100, 10, 5) == -3 and b"512" in lib.rtk_last_error_string()
    assert call(f32, 36, 100, 1, 100, 10, 5) == -1 and b"block" in lib.rtk_last_error_string()
    assert call(f32, 36, 100, 0, 100, 10, 5, ws_bytes=1024) == -1 and b"workspace" in lib.rtk_last_error_string()
    assert call(f32, 36, 100, 0, 100, 10, 5, slot=a) == -1 and b"CSR" in lib.rtk_last_error_string()
    assert lib.rtk_score_topk_f32(None, 4, 36, a, 100, 0, 100, None, None, None, None, 10, 5, a, a, a, 1 << 30, None) == -1
    assert lib.rtk_score_topk_f32(a, 0, 36, a, 100, 0, 100, None, None, None, None, 10, 5, a, a, a, 1 << 30, None) == 0


# ---- the algorithm in numpy ---------------------------------------------------------------------------------------

def sel_key(x):
    """The select kernel's key (csrc/rtk_topk_key.h): integer order = candidate order; every NaN one key above +inf,
    -0 -> +0."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where((u & 0x7fffffff) > 0x7f800000, 0x7fc00000, u)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000).astype(np.int64)


KEY_NINF = int(sel_key(np.float32("-inf")))


def eligible(N, objs, keep):
    e = np.ones(N, dtype=bool)
    for o in objs:
        if 0 <= o < N and o != keep:
            e[o] = False
    return e


def plain_topk(p, k, objs, keep):
    """stable descending sort of the eligible entries, cut at k, padded with -1"""
    key = sel_key(p)
    idx = np.flatnonzero(eligible(len(p), objs, keep))
    order = idx[np.lexsort((idx, -key[idx]))][:k]
    return order.tolist() + [-1] * (k - len(order))


def select(keys, ids, k):
    """rtk_select_topk's rule on one row in merge mode: the keys above the cut-off key K*, then the first ones equal
    to K* in COLUMN order, sorted by (key descending, id ascending)."""
    cols = np.flatnonzero(ids >= 0)
    kp = min(k, len(cols))
    if kp == 0:
        return [-1] * k
    kstar = np.sort(keys[cols])[::-1][kp - 1]
    above = cols[keys[cols] > kstar]
    tied = cols[keys[cols] == kstar][: kp - len(above)]
    take = np.concatenate([above, tied])
    take = take[np.lexsort((ids[take], -keys[take]))]
    return ids[take].tolist() + [-1] * (k - kp)


def stream_topk(p, k, objs, keep, col0=0, patch=True):
    """steps 1-5 on one query and one block p = the probabilities of entities [col0, col0 + len(p))"""
    n = len(p)
    key = sel_key(p)
    elig = eligible(n, [o - col0 for o in objs], keep - col0 if keep >= 0 else -1)
    n_tiles = -(-n // TILE)
    tmax = np.full(n_tiles, KEY_NINF, dtype=np.int64)
    for t in range(n_tiles):                                     # step 1: maxima over all rows of the tile ...
        tmax[t] = key[t * TILE:(t + 1) * TILE].max()
    if patch:
        for o in objs:                                           # step 2: ... corrected where a filtered object lies
            j = o - col0
            if 0 <= j < n and o != keep:
                t = j // TILE
                seg = key[t * TILE:(t + 1) * TILE][elig[t * TILE:(t + 1) * TILE]]
                tmax[t] = seg.max() if len(seg) else KEY_NINF
    k_t = min(k, n_tiles)
    tiles = np.lexsort((np.arange(n_tiles), -tmax))[:k_t]        # step 3: best tiles, ties by lower tile
    ck, ci = [], []
    for t in np.sort(tiles):                                     # step 4: candidates in ascending id order
        for j in range(t * TILE, (t + 1) * TILE):
            ok = j < n and elig[j]
            ck.append(key[j] if ok else KEY_NINF)
            ci.append(col0 + j if ok else -1)
    return select(np.asarray(ck), np.asarray(ci), k)             # step 5


def cases():
    rng = np.random.default_rng(0)
    levels = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    for N in (1, 127, 128, 129, 300, 1000, 1500):
        for k in (1, 3, 10, 128):
            for trial in range(6):
                p = levels[rng.integers(0, 3, N)]                # heavy ties: three levels
                if trial % 3 == 1:
                    p[rng.integers(0, N, max(1, N // 50))] = np.nan
                if trial % 3 == 2:
                    p[rng.integers(0, N, max(1, N // 100))] = np.float32(0.9)     # a few clear winners
                best = np.flatnonzero(sel_key(p) == sel_key(p).max())
                objs = rng.choice(best, size=min(len(best), int(rng.integers(0, 40))), replace=False).tolist()   # hit the best tiles
                objs += rng.integers(0, N + 10, int(rng.integers(0, 30))).tolist()                               # some out of range
                if trial == 5:
                    objs = list(range(N))[: max(0, N - 2)]       # fewer than k left
                keep = int(objs[0]) if objs and trial % 2 else -1
                yield p, k, objs, keep


def test_lemma_and_tie_rule_against_a_plain_sort():
    n = 0
    for p, k, objs, keep in cases():
        assert stream_topk(p, k, objs, keep) == plain_topk(p, k, objs, keep)
        n += 1
    assert n > 100


def test_blocks_merge_to_the_whole_range():
    for p, k, objs, keep in cases():
        N = len(p)
        if N < 129:
            continue
        whole = plain_topk(p, k, objs, keep)
        for cuts in ((0, 1, N), (0, 130, 131, N), (0, N // 2 + 3, N)):
            ids = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ids += stream_topk(p[lo:hi], k, objs, keep, col0=lo)
            ids = np.asarray(ids)
            keys = np.where(ids >= 0, sel_key(p)[np.maximum(ids, 0)], KEY_NINF)
            assert select(keys, ids, k) == whole


def test_unpatched_maxima_choose_the_wrong_tiles():
    """Why step 2 exists: the filtered best entity of a tile must not speak for it."""
    p = np.full(3 * TILE, 0.25, dtype=np.float32)
    p[5] = 0.9                                  # filtered: tile 0 has nothing else to offer
    p[TILE + 1] = p[2 * TILE + 1] = 0.5
    assert plain_topk(p, 1, [5], -1) == [TILE + 1]
    assert stream_topk(p, 1, [5], -1) == [TILE + 1]
    assert stream_topk(p, 1, [5], -1, patch=False) != [TILE + 1]
    assert stream_topk(p, 1, [5], 5) == [5]     # keep_idx keeps it
