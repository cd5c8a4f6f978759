"""The ordered scatter (gO of ``rtk_score_candidates_bwd_*``): cases, a float64 reference and a bit-exact float32
emulation of the order in which the kernels add.

The order, read from the kernels (sort, windowed run sum, combine):

  * entry i = d K + k has the key cand[d, k]; a key outside [0, n_ent) becomes n_ent and sorts last;
  * the sort is stable: ascending i within an entity (a *run* = the sorted entries of one entity);
  * window w owns the sorted positions [w win, (w + 1) win), win = cand_window(M);
  * inside a window a run starts from 0 and adds fmaf(dz[i], v[d, col], acc) in sorted order, per column;
  * a run inside one window is stored as it is; a run over several windows is the partial of the window where it
    starts plus the partials of the following windows, in window order, by plain float32 adds;
  * rows without entries and invalid keys give zeros.

dz and v carry at most 12 significant bits (``exact_cases.round_mantissa``), so every product is a float32 number
and fmaf(dz, v, acc) is ONE correctly rounded float32 add: the emulation is a chain of ``np.float32`` adds and has to
equal the kernels' gO bit for bit.  Exponents are spread over 2^-8 .. 2^8 per factor, so that nearly every add
rounds and an order change shows in the bits (``tests/test_scatter_cases_host.py`` proves that with four mutants).

A case plants its runs by length: ``runs`` are the lengths of the runs in ascending entity order, so a run's sorted
positions -- and which windows it touches -- are fixed by the lengths before it; the entries are then dealt to the
(d, k) slots in a random order, which the stable sort has to undo.  ``tail`` random runs fill M = B K, ``bad``
invalid ids (negative and >= n_ent alternating) sort behind the last valid run.

Host-only (numpy).
"""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

from exact_cases import gamma, round_mantissa

SENTINEL = np.float32(-7.0e30)      # dz padding (ld_dz > K): a kernel that reads it changes every sum it enters
WIN_MAX, MAXC = 256, 1024
LABELS = frozenset({
    "inside", "two_windows", "three_plus", "ends_on_window_end", "starts_on_window_start", "both_slots",
    "last_window_partial", "last_window_full", "single_entry", "negative_id", "large_id", "run_before_invalid",
    "unnamed_entity", "unroll8_tail", "unroll4_tail", "win32", "shared_list", "wide_dz", "v_offset", "go_offset",
    "no_vector", "radix1", "radix2", "radix3", "empty",
})


def cand_window(M):
    """Entries per wave of the run sum: M / 4096 rounded up to a multiple of 16, within [16, 256]."""
    w = -(-(-(-M // 4096)) // 16) * 16
    return min(max(w, 16), WIN_MAX)


def radix_passes(n_ent):
    bits = 1
    while (n_ent >> bits) != 0:
        bits += 1
    return -(-bits // 8)


@dataclass(frozen=True)
class ScatterCase:
    """gO (n_ent x c) of a (B, K) candidate matrix.  shared: ld_cand = 0, one list for every query.  dz_pad /
    cand_pad: ld - K (padding holds SENTINEL / the valid id 0).  v_off / go_off: floats off a 16-byte boundary."""
    name: str
    B: int
    K: int
    c: int
    n_ent: int
    runs: tuple = ()
    mean: int = 9
    bad: int = 0
    shared: bool = False
    dz_pad: int = 0
    cand_pad: int = 0
    v_off: int = 0
    go_off: int = 0

    @property
    def M(self):
        return self.B * self.K

    @property
    def win(self):
        return cand_window(self.M)


def _case(name, B, K, c, n_ent, **kw):
    return ScatterCase(name, B, K, c, n_ent, **kw)


# Planted run lengths at win = 16 (sorted positions in brackets): 5 [0, 5) inside; 11 [5, 16) ends on a window's last
# position; 16 [16, 32) a whole window of its own; 3 [32, 35); 20 [35, 55) two windows; 50 [55, 105) four windows, so
# window 3 holds the tail of one crossing run and the head of the next (slot 0 and slot 1) and windows 4, 5 hold
# slot-0 partials alone; 7 [105, 112) ends on a window's end; 40 [112, 152) starts on a window's first position behind
# another key and covers three windows; 2 [152, 154) a valid run directly before the invalid ids.
PLANTED = (5, 11, 16, 3, 20, 50, 7, 40, 2)

CASES = (
    _case("single", 1, 1, 4, 255),
    _case("planted_c6", 53, 3, 6, 255, runs=PLANTED, bad=5),                 # M = 159: 154 planted + 5 invalid
    _case("planted_c4", 53, 3, 4, 255, runs=PLANTED, bad=5),
    _case("full_last_window", 16, 10, 4, 255, runs=(40, 24), mean=7),        # M = 160 = 10 windows
    _case("c256", 61, 5, 256, 300, runs=(37,), mean=11),                     # M = 305
    _case("c260", 61, 5, 260, 300, runs=(37,), mean=11),
    _case("c516", 43, 7, 516, 300, runs=(37,), mean=11, bad=3),              # M = 301: not a multiple of 4
    _case("c1024", 43, 7, 1024, 300, runs=(70,), mean=11),
    _case("v_offset", 61, 5, 8, 300, runs=(37,), v_off=1),
    _case("go_offset", 61, 5, 8, 300, runs=(37,), go_off=1),
    _case("m1023", 1023, 1, 4, 256, bad=2),
    _case("m1024", 32, 32, 4, 256),
    _case("m1025", 25, 41, 4, 256, bad=1),
    _case("n255", 70, 30, 4, 255, mean=14, bad=4),                           # one radix pass
    _case("n256", 70, 30, 4, 256, mean=14, bad=4),                           # two: the key n_ent needs bit 8
    _case("n65535", 70, 30, 4, 65535, mean=14, bad=4),                       # two
    _case("n65536", 70, 30, 4, 65536, mean=14, bad=4),                       # three
    _case("shared_list", 40, 9, 12, 300, shared=True, bad=2),                # every entity of the list: a run of 40
    _case("wide_dz", 37, 11, 20, 300, runs=(45,), dz_pad=3, cand_pad=2, bad=3),
    _case("win32", 1040, 64, 4, 5000, runs=(7, 25, 32, 70, 100, 3), mean=24, bad=6),     # M = 66 560
    _case("empty_batch", 0, 5, 8, 40),
    _case("empty_k", 4, 0, 8, 40),
)
BF16_CASE = "planted_c6"            # the one case that also runs with a bf16 O: the same bits, gO never reads O
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------- operands -----
def _values(rng, shape):
    x = rng.standard_normal(shape) * 2.0 ** rng.uniform(-8, 8, shape)
    x = round_mantissa(x, 12)
    assert np.all(x != 0) and np.all(np.abs(x) > 2.0 ** -40) and np.all(np.abs(x) < 2.0 ** 24)
    return x


def _run_lengths(case, rng):
    """The valid runs' lengths in ascending entity order: the planted ones, then random ones up to M - bad."""
    left = case.M - case.bad - sum(case.runs)
    assert left >= 0, case.name
    runs = list(case.runs)
    while left > 0:
        n = min(int(rng.geometric(1.0 / case.mean)), left)
        runs.append(n)
        left -= n
    assert len(runs) < case.n_ent, f"{case.name}: more runs than entities (one entity stays unnamed)"
    return runs


def _bad_ids(case):
    pool = [-1, case.n_ent, -(2 ** 40), case.n_ent + 5, 10 ** 12, -3]
    return [pool[i % len(pool)] for i in range(case.bad)]


@functools.lru_cache(maxsize=None)
def operands(case):
    """-> cand (B or 1, K + cand_pad) int64, dz (B, K + dz_pad) float32, v (B, c) float32.  Read-only."""
    rng = np.random.default_rng(zlib.crc32(("scatter " + case.name).encode()))
    B, K, M = case.B, case.K, case.M
    if case.shared:
        ids = np.sort(rng.choice(case.n_ent, K - case.bad, replace=False)).tolist() + _bad_ids(case)
        cand = np.array(ids, dtype=np.int64)[rng.permutation(K)][None, :]
    else:
        runs = _run_lengths(case, rng)
        ents = np.sort(rng.choice(case.n_ent - 2, len(runs), replace=False)) + 1 if runs else np.zeros(0, np.int64)
        if len(runs) >= 2:
            ents[0], ents[-1] = 0, case.n_ent - 1                            # the first and the last row of gO
        flat = np.concatenate([np.repeat(ents, runs), np.array(_bad_ids(case), dtype=np.int64)]).astype(np.int64)
        assert flat.size == M
        cand = np.zeros((B, K + case.cand_pad), dtype=np.int64)             # padding: the valid id 0
        cand[:, :K] = flat[rng.permutation(M)].reshape(B, K)
    dz = np.full((B, K + case.dz_pad), SENTINEL, dtype=np.float32)
    dz[:, :K] = _values(rng, (B, K))
    v = _values(rng, (B, case.c))
    for a in (cand, dz, v):
        a.setflags(write=False)
    return cand, dz, v


def keys_of(case, cand):
    """The sort key of every entry i = d K + k."""
    ids = np.broadcast_to(cand[:, :case.K], (case.B, case.K)).reshape(-1)
    return np.where((ids >= 0) & (ids < case.n_ent), ids, case.n_ent)


def sorted_runs(case, cand, descending=False):
    """-> order (entry at every sorted position), [(entity, first position, end position)] of the valid runs."""
    keys = keys_of(case, cand)
    idx = np.arange(keys.size)
    order = np.lexsort((-idx if descending else idx, keys))
    skey = keys[order]
    cuts = np.flatnonzero(np.diff(skey)) + 1
    starts = np.concatenate([[0], cuts]) if skey.size else np.zeros(0, np.int64)
    ends = np.concatenate([cuts, [skey.size]]) if skey.size else np.zeros(0, np.int64)
    return order, [(int(skey[s]), int(s), int(e)) for s, e in zip(starts, ends) if skey[s] < case.n_ent]


# ---------------------------------------------------------------------------------- reference, emulation -----
@functools.lru_cache(maxsize=None)
def reference(case):
    """-> gO in float64, and per row the bound gamma(n - 1) sum |dz v| of ANY order of float32 adds over the row's n
    exact products (n - 1 adds lie on the longest path of any summation tree; the first fmaf onto 0 is exact)."""
    cand, dz, v = operands(case)
    g = np.zeros((case.n_ent, case.c))
    a = np.zeros((case.n_ent, case.c))
    order, runs = sorted_runs(case, cand)
    for e, s, t in runs:
        i = order[s:t]
        d, k = i // case.K, i % case.K
        terms = dz[d, k].astype(np.float64)[:, None] * v[d].astype(np.float64)
        g[e] = terms.sum(0)
        a[e] = gamma(t - s - 1) * np.abs(terms).sum(0)
    return g, a


def emulate(case, win=None, descending=False, reverse_combine=False, carry=False):
    """gO in the kernels' order, float32.  The keyword arguments are the mutants: another window, descending entry
    order inside an entity, the window partials added last to first, the chain carried across window boundaries."""
    cand, dz, v = operands(case)
    win = win or case.win
    gO = np.zeros((case.n_ent, case.c), dtype=np.float32)
    order, runs = sorted_runs(case, cand, descending)
    zero = np.zeros(case.c, dtype=np.float32)
    for e, s, t in runs:
        parts, acc = [], zero
        for p in range(s, t):
            if p > s and p % win == 0 and not carry:
                parts.append(acc)
                acc = zero
            d, k = divmod(int(order[p]), case.K)
            prod = dz[d, k] * v[d]                      # exact: 12 x 12 significant bits
            acc = acc + prod                            # fmaf with an exact product: one rounding
            assert acc.dtype == np.float32
        parts.append(acc)
        if reverse_combine:
            parts.reverse()
        tot = parts[0]
        for q in parts[1:]:
            tot = tot + q
        gO[e] = tot
    return gO


@functools.lru_cache(maxsize=None)
def expected(case):
    g = emulate(case)
    g.setflags(write=False)
    return g


MUTANTS = {
    "window twice as long": lambda case: emulate(case, win=2 * case.win),
    "descending i within an entity": lambda case: emulate(case, descending=True),
    "combine order reversed": lambda case: emulate(case, reverse_combine=True),
    "chain carried across windows": lambda case: emulate(case, carry=True),
}


# ---------------------------------------------------------------------------------------------- coverage -----
def features(case):
    """What of LABELS the case reaches, from its sorted keys and its window."""
    f = set()
    M, win = case.M, case.win
    if M == 0:
        return {"empty"}
    cand, _, _ = operands(case)
    _, runs = sorted_runs(case, cand)
    ids = np.broadcast_to(cand[:, :case.K], (case.B, case.K))
    tails, heads = set(), set()                         # windows holding the end / the start of a crossing run
    for e, s, t in runs:
        w0, w1 = s // win, (t - 1) // win
        f.add("inside" if w0 == w1 else "two_windows" if w1 == w0 + 1 else "three_plus")
        if t % win == 0 and t < M:
            f.add("ends_on_window_end")
        if s % win == 0 and s > 0:
            f.add("starts_on_window_start")
        if w1 > w0:
            heads.add(w0)
            tails.add(w1)
    if tails & heads:
        f.add("both_slots")
    f.add("last_window_partial" if M % win else "last_window_full")
    if M == 1:
        f.add("single_entry")
    if (ids < 0).any():
        f.add("negative_id")
    if (ids >= case.n_ent).any():
        f.add("large_id")
    if runs and runs[-1][2] < M:
        f.add("run_before_invalid")
    if len(runs) < case.n_ent:
        f.add("unnamed_entity")
    if case.c <= 512 and M % 8:
        f.add("unroll8_tail")
    if case.c > 512 and M % 4:
        f.add("unroll4_tail")
    if win == 32:
        f.add("win32")
    if case.shared:
        f.add("shared_list")
    if case.dz_pad:
        f.add("wide_dz")
    if case.v_off % 4:
        f.add("v_offset")
    if case.go_off % 4:
        f.add("go_offset")
    if case.c % 4:
        f.add("no_vector")
    f.add(f"radix{radix_passes(case.n_ent)}")
    return f
