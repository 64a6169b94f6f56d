"""Retrieval evaluation on the device: recall@k, NDCG@k and hit rate of user-to-item (u2i) and item-to-item (i2i)
retrieval over an embedding table, the step that follows training a link-prediction / recommendation model
(examples/train_sage_unsup.py, examples/train_node2vec.py produce such tables).

The embeddings here are synthetic with PLANTED neighbours: items come in groups of `group` siblings around a centre on an
integer lattice, a user sits next to one centre, and the ground truth of a user (or of an item) is the group.  Every
coordinate is a small multiple of 1/8, so every score is exact in float32 and in float64 alike: the search's ids can be
compared with a float64 brute force without a tolerance, ties included (both break them by row).

The search is glx.Features.search on the item table as it lies in device memory (exact, deterministic: one fmaf chain per
score, ties to the smaller row); the metrics are computed on the device from its ids.  Planted groups are what the L2
metric retrieves; under the inner product long items win regardless of the group, which the lower numbers show.

--index ivf also builds an IVF-Flat index over the item table (glx.Features.build_ivf, --nlist lists) and repeats every
search through it with --nprobe lists probed: one more line per search with the index's own metrics and its recall
against the exact search's ids.  The index scores rows from the same table with the same chain, so what it returns are
exact distances; what it can miss are rows in lists it did not probe.

--index ivfpq builds an IVF-PQ index on top of that one (glx.KnnIvf.build_pq, --m sub-quantisers of 256 codewords) and
adds a third line per search next to the IVF-Flat one: the probed lists are scanned through --m bytes of codes per row,
and the --refine best candidates by the coded score are re-scored from the table (--refine 0 returns the coded ranking
itself).  With --refine > 0 the distances it returns are exact too; what it can miss in addition are rows the coded score
ranked below the first --refine.

--dtype bfloat16 | float16 | float8_e4m3fn | float8_e5m2 also stores the item table in that type (rounded on the device
while it is uploaded) and adds one line per search: the exact search on the narrow table, its metrics and its recall
against the float32 table's answer -- what the rounding of the stored rows costs; the queries stay float32.

Exits non-zero unless two runs give the same bits and the ids equal the float64 brute force (with --index ivf or ivfpq:
and two index searches give the same bits, and the index with every list probed equals the exact search bit for bit;
with --index ivfpq and --refine > 0: and every distance the coded index returns is the exact search's for that id).
Usage: python examples/eval_recall.py [--items 4000] [--users 1000] [--dim 16] [--k 10]
                                      [--index flat|ivf|ivfpq] [--nlist 64] [--nprobe 4] [--m 4] [--refine 100]
                                      [--dtype float32|bfloat16|float16|float8_e4m3fn|float8_e5m2]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import glx  # noqa: E402


def planted(rng, num_items, num_users, dim, group):
    groups = num_items // group
    centre = rng.integers(-8, 9, (groups, dim)).astype(np.float32)
    items = np.repeat(centre, group, axis=0)
    for j in range(group):  # sibling j leaves the centre along axis j by (j + 1) / 4
        items[j::group, j % dim] += 0.25 * (j + 1)
    item_ids = (10 ** 6 + 3 * rng.permutation(groups * group)).astype(np.int64)  # node ids, not row numbers
    user_group = rng.integers(0, groups, num_users)
    users = centre[user_group] + rng.integers(-1, 2, (num_users, dim)).astype(np.float32) / 8
    return items, item_ids, users, user_group


def brute64(q, x, k, metric):
    q, x = q.astype(np.float64), x.astype(np.float64)
    s = -(q @ x.T) if metric == "ip" else (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * (q @ x.T)
    return np.argsort(s, axis=1, kind="stable")[:, :k]


def metrics(ids, truth, k):
    """ids[n, k], truth[n, t] (device): recall@k, NDCG@k, hit rate"""
    hit = (ids[:, :, None] == truth[:, None, :]).any(2)
    disc = 1.0 / torch.log2(torch.arange(k, device=ids.device, dtype=torch.float32) + 2.0)
    ideal = disc[:min(k, truth.shape[1])].sum()
    recall = hit.sum(1).float() / min(k, truth.shape[1])
    ndcg = (hit.float() * disc).sum(1) / ideal
    return recall.mean().item(), ndcg.mean().item(), hit.any(1).float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4000)
    ap.add_argument("--users", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--index", choices=("flat", "ivf", "ivfpq"), default="flat")
    ap.add_argument("--nlist", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=4)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--refine", type=int, default=100)
    ap.add_argument("--dtype", choices=sorted(dict(glx.FEATURE_DTYPES, **glx.FP8_FEATURE_DTYPES)), default="float32")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    items, item_ids, users, user_group = planted(rng, a.items, a.users, a.dim, a.group)
    table = glx.Features(items, ids=item_ids)
    narrow = glx.Features(items, ids=item_ids, dtype=a.dtype) if a.dtype != "float32" else None
    index = table.build_ivf(a.nlist) if a.index in ("ivf", "ivfpq") else None
    coded = index.build_pq(a.m) if a.index == "ivfpq" else None
    d_ids = torch.from_numpy(item_ids).cuda()
    group_rows = torch.arange(items.shape[0], device="cuda").view(-1, a.group)
    ok = True
    for task, q, q_group in (("u2i", users, user_group), ("i2i", items, np.arange(items.shape[0]) // a.group)):
        dq = torch.from_numpy(q).cuda()
        truth = d_ids[group_rows[torch.from_numpy(q_group).cuda()]]
        for metric in ("l2", "ip"):
            ids, dist = table.search(dq, a.k, metric)
            ids2, dist2 = table.search(dq, a.k, metric)
            same_bits = bool(torch.equal(ids, ids2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32)))
            want = item_ids[brute64(q, items, a.k, metric)]
            exact = bool(np.array_equal(ids.cpu().numpy(), want))
            r, n, h = metrics(ids, truth, a.k)
            print("%s %s  recall@%d %.4f  ndcg@%d %.4f  hit rate %.4f  two runs same bits: %s  ids == float64 brute force: %s"
                  % (task, metric, a.k, r, a.k, n, h, same_bits, exact))
            ok = ok and same_bits and exact and not math.isnan(r)
            if narrow is not None:
                nids, ndist = narrow.search(dq, a.k, metric)
                nids2, ndist2 = narrow.search(dq, a.k, metric)
                same_bits = bool(torch.equal(nids, nids2) and torch.equal(ndist.view(torch.int32), ndist2.view(torch.int32)))
                r, n, h = metrics(nids, truth, a.k)
                vs_f32 = (nids[:, :, None] == ids[:, None, :]).any(1).float().mean().item()
                print("%s %s  table stored as %s  recall@%d %.4f  ndcg@%d %.4f  hit rate %.4f  recall vs float32 table %.4f  "
                      "two runs same bits: %s" % (task, metric, a.dtype, a.k, r, a.k, n, h, vs_f32, same_bits))
                ok = ok and same_bits
            if index is None:
                continue
            got, gdist = index.search(dq, a.k, metric, nprobe=a.nprobe)
            got2, gdist2 = index.search(dq, a.k, metric, nprobe=a.nprobe)
            same_bits = bool(torch.equal(got, got2) and torch.equal(gdist.view(torch.int32), gdist2.view(torch.int32)))
            full, fdist = index.search(dq, a.k, metric, nprobe=a.nlist)
            all_lists = bool(torch.equal(full, ids) and torch.equal(fdist.view(torch.int32), dist.view(torch.int32)))
            r, n, h = metrics(got, truth, a.k)
            vs_flat = (got[:, :, None] == ids[:, None, :]).any(1).float().mean().item()
            print("%s %s  ivf nlist %d nprobe %d  recall@%d %.4f  ndcg@%d %.4f  hit rate %.4f  recall vs exact %.4f  "
                  "two runs same bits: %s  every list probed == exact search: %s"
                  % (task, metric, a.nlist, a.nprobe, a.k, r, a.k, n, h, vs_flat, same_bits, all_lists))
            ok = ok and same_bits and all_lists
            if coded is None:
                continue
            pids, pdist = coded.search(dq, a.k, metric, nprobe=a.nprobe, refine=a.refine)
            pids2, pdist2 = coded.search(dq, a.k, metric, nprobe=a.nprobe, refine=a.refine)
            same_bits = bool(torch.equal(pids, pids2) and torch.equal(pdist.view(torch.int32), pdist2.view(torch.int32)))
            r, n, h = metrics(pids, truth, a.k)
            vs_flat = (pids[:, :, None] == ids[:, None, :]).any(1).float().mean().item()
            vs_ivf = ((pids[:, :, None] == got[:, None, :]) & (got[:, None, :] >= 0)).any(1).float().mean().item()
            print("%s %s  ivfpq nlist %d nprobe %d m %d refine %d  recall@%d %.4f  ndcg@%d %.4f  hit rate %.4f  "
                  "recall vs exact %.4f (ivf %.4f)  recall vs ivf %.4f  two runs same bits: %s"
                  % (task, metric, a.nlist, a.nprobe, a.m, a.refine, a.k, r, a.k, n, h, vs_flat,
                     (got[:, :, None] == ids[:, None, :]).any(1).float().mean().item(), vs_ivf, same_bits), end="")
            ok = ok and same_bits
            if a.refine > 0:  # re-ranked distances are the exact search's: look each returned id up in a full search
                all_ids, all_dist = table.search(dq, min(items.shape[0], 1024), metric)
                at = (pids[:, :, None] == all_ids[:, None, :])
                found = at.any(2) & (pids >= 0)
                exact_d = (at.float() * torch.nan_to_num(all_dist)[:, None, :]).sum(2)
                same_d = bool(torch.equal(exact_d[found], torch.nan_to_num(pdist)[found]))
                print("  returned distances == exact search's: %s" % same_d, end="")
                ok = ok and same_d
            print()
    if not ok:
        print("FAILED")
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
