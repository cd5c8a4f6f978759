"""What the cross-entropy tests share (a plain module, no fixtures): the synthetic pair table of
test_gpu_loss_stream.py and the float64 reference of ``ce_loss_1vN`` -- ``oracle.score_oracle.logits_ref`` on float64
parameters with autograd, then ``F.cross_entropy(z, y)`` with the targets of the definition."""
import numpy as np
import torch

from oracle import score_oracle as orc


class Pairs:
    """The attributes DeviceFilter reads from a KG_dataset, for a synthetic (pair -> objects) table."""
    def __init__(self, pairs, lists, n_ent, eps):
        self._pair_slot = {p: i for i, p in enumerate(pairs)}
        self._ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        self._obj = np.asarray([x for l in lists for x in l], dtype=np.int64)
        self.features = np.asarray(pairs, dtype=np.int64)
        self.n_ent, self.label_smoothing = n_ent, eps

    def objects(self, i):
        """The objects of pair i, each once (as DeviceFilter holds them)."""
        return np.unique(self._obj[self._ptr[i]:self._ptr[i + 1]])

    def targets(self, ids, eps):
        """y[d, j] = (1 - eps) [j in P_d] / n_d + eps / N, float64."""
        y = torch.full((len(ids), self.n_ent), eps / self.n_ent, dtype=torch.float64)
        for row, i in enumerate(ids):
            objs = self.objects(i)
            if len(objs):
                y[row, torch.from_numpy(objs)] += (1.0 - eps) / len(objs)
        return y


def batch(n_ent, n_rel, B, seed, eps, max_len=9, empty=False, n_pairs=200):
    """A synthetic pair table and a batch of B of its items (with repeats when there are fewer pairs than B)."""
    rng = np.random.default_rng(seed)
    n_pairs = min(n_pairs, n_ent)
    pairs = [(int(s), int(r)) for s, r in zip(rng.permutation(n_ent)[:n_pairs], rng.integers(0, n_rel, n_pairs))]
    lists = [rng.integers(0, n_ent, rng.integers(1, max_len)).tolist() for _ in pairs]
    lists[min(3, n_pairs - 1)] = lists[min(3, n_pairs - 1)] * 2          # repeated triples: every object counts once
    ids = rng.permutation(n_pairs)[:B] if B <= n_pairs else rng.integers(0, n_pairs, B)
    if empty:
        lists[int(ids[0])] = []                                          # a query without known objects
    return Pairs(pairs, lists, n_ent, eps), np.asarray(ids, dtype=np.int64)


def ce_ref(core, R, S, O, h, r, y, shared=False):
    """(loss, g_core, g_R, g_S[, g_O], max |z|) in float64: autograd through logits_ref and F.cross_entropy."""
    ps = [torch.as_tensor(x).detach().double().clone().requires_grad_(True) for x in (core, R, S)]
    if not shared:
        ps.append(torch.as_tensor(O).detach().double().clone().requires_grad_(True))
    z = orc.logits_ref(ps[0], ps[1], ps[2], ps[2] if shared else ps[3], h, r)
    loss = torch.nn.functional.cross_entropy(z, y)
    loss.backward()
    return [loss.detach()] + [p.grad for p in ps] + [z.detach().abs().max().item()]
