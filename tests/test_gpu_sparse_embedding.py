"""graphlearn.nn.pytorch.SparseEmbedding and the Sparse* optimizers: the torch surface of glx_rows_coalesce and
glx_embedding_update, against the numpy restatement (embedding_ref.py) bit for bit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import embedding_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-learn_amd", "python"))

pytestmark = pytest.mark.gpu

V, D = 29, 12
LR = 0.05


@pytest.fixture(scope="module")
def thg():
    import graphlearn.nn.pytorch as m
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _grad(rng, shape):
    """magnitudes in [2^-10, 2^3], signed, never a zero of either sign"""
    return (np.exp2(rng.uniform(-10.0, 3.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _make(thg, algo, emb):
    if algo == eref.SGD:
        return thg.SparseSGD(emb, lr=LR)
    if algo == eref.ADAGRAD:
        return thg.SparseAdagrad(emb, lr=LR)
    return thg.SparseAdam(emb, lr=LR)


def _ref_scalars(algo, t):
    if algo == eref.ADAM:
        return eref.adam_scalars(LR, (0.9, 0.999), 1e-8, t)
    return (LR, 1e-10 if algo == eref.ADAGRAD else 0.0, 0.0, 0.0, 0.0, 0.0)


def _ref_states(algo):
    return [np.zeros((V, D), np.float32) for _ in range({eref.SGD: 0, eref.ADAGRAD: 1}.get(algo, 2))] + [None, None]


def _ref_step(algo, W, states, ids, g, t, coalesce=True):
    if coalesce:
        ids, g, _ = eref.coalesce(ids, g, W.shape[0])
    eref.update(algo, W, ids, g, states[0], states[1], *_ref_scalars(algo, t))


def test_forward_is_the_rows_of_the_weight_and_zeros_outside(thg):
    import torch
    emb = thg.SparseEmbedding(V, D, seed=3)
    assert emb.weight.shape == (V, D) and emb.weight.is_cuda and emb.weight.dtype == torch.float32
    assert not list(emb.parameters()) and "weight" in emb.state_dict() and not emb.weight.requires_grad
    assert torch.equal(emb.weight, thg.SparseEmbedding(V, D, seed=3).weight)  # the seed decides the values
    assert not torch.equal(emb.weight, thg.SparseEmbedding(V, D, seed=4).weight)
    ids = _cuda(np.array([[0, V - 1, 5], [5, -1, V]], np.int64))
    out = emb(ids)
    assert out.shape == (2, 3, D) and out.grad_fn is not None
    want = emb.weight[ids.clamp(0, V - 1)].clone()
    want[1, 1:] = 0.0
    assert np.array_equal(_bits(out), _bits(want))
    with torch.no_grad():
        assert np.array_equal(_bits(emb(ids)), _bits(want))


def test_backward_notes_row_gradients_and_builds_no_table_sized_tensor(thg):
    import torch
    emb = thg.SparseEmbedding(V, D)
    a, b = _cuda(np.array([1, 2, 2], np.int64)), _cuda(np.array([[2, 3]], np.int64))
    ca, cb = _cuda(np.ones((3, D), np.float32)), _cuda(np.full((1, 2, D), 2.0, np.float32))
    loss = (emb(a) * ca).sum() + (emb(b, distinct=True) * cb).sum()
    loss.backward()
    assert emb.weight.grad is None and emb._anchor.grad is None
    assert len(emb._pending) == 2
    by_seq = sorted(emb._pending, key=lambda e: e[0])
    assert [e[0] for e in by_seq] == [1, 2] and [e[3] for e in by_seq] == [False, True]
    assert by_seq[0][1].tolist() == [1, 2, 2] and by_seq[1][1].tolist() == [2, 3]
    assert tuple(by_seq[0][2].shape) == (3, D) and tuple(by_seq[1][2].shape) == (2, D)
    assert torch.equal(by_seq[1][2], cb.view(2, D))


@pytest.mark.parametrize("forwards", [1, 2], ids=["one_forward", "two_overlapping_forwards"])
@pytest.mark.parametrize("algo", [eref.SGD, eref.ADAGRAD, eref.ADAM])
def test_three_steps_equal_the_restatement(thg, algo, forwards):
    """the whole table and the state tables after each step: the restatement's coalesce + update over the pending
    gradients concatenated in forward order; ids repeat inside a forward, across forwards, and fall outside the table"""
    rng = np.random.default_rng(10 * algo + forwards)
    emb = thg.SparseEmbedding(V, D, seed=algo)
    opt = _make(thg, algo, emb)
    W, states = emb.weight.cpu().numpy().copy(), _ref_states(algo)
    for t in range(1, 4):
        ids = [rng.integers(-1, V + 1, shape).astype(np.int64) for shape in ((9,), (4, 3))[:forwards]]
        ids[0][:3] = 7
        if forwards == 2:
            ids[1][0, 0], ids[1][1, 1] = 7, ids[0][5]
        coef = [_grad(rng, i.shape + (D,)) for i in ids]
        opt.zero_grad()
        outs = [emb(_cuda(i)) for i in ids]
        # the second forward's term first: the order backward runs in is not the order of the forwards
        loss = sum((o * _cuda(c)).sum() for o, c in reversed(list(zip(outs, coef))))
        loss.backward()
        assert len(emb._pending) == forwards
        opt.step()
        assert emb._pending == []
        _ref_step(algo, W, states, np.concatenate([i.reshape(-1) for i in ids]),
                  np.concatenate([c.reshape(-1, D) for c in coef]), t)
        assert np.array_equal(_bits(emb.weight), W.view(np.uint32)), (algo, forwards, t)
        for key, s in zip(("state1", "state2"), states):
            if s is not None:
                assert np.array_equal(_bits(opt.state[0][key]), s.view(np.uint32)), (algo, forwards, t, key)
    assert opt.state[0]["step"] == 3


@pytest.mark.parametrize("algo", [eref.SGD, eref.ADAGRAD, eref.ADAM])
def test_the_distinct_path_equals_the_coalesced_path(thg, algo):
    """distinct ids (one out of range), gradients without a zero: the direct path skips the coalesce and gives the same
    bits.  (With a -0.0 element the two could differ in the sign of a zero: the coalesce adds every term to +0.0, which
    turns -0.0 into +0.0; the direct path hands the element on as it is.)"""
    rng = np.random.default_rng(40 + algo)
    embs = [thg.SparseEmbedding(V, D, seed=9) for _ in range(2)]
    opts = [_make(thg, algo, e) for e in embs]
    W, states = embs[0].weight.cpu().numpy().copy(), _ref_states(algo)
    for t in range(1, 3):
        ids = rng.permutation(V + 1)[:11].astype(np.int64)  # V itself may be among them: outside the table
        ids[4] = V
        coef = _grad(rng, (11, D))
        for emb, opt, distinct in zip(embs, opts, (True, False)):
            (emb(_cuda(ids), distinct=distinct) * _cuda(coef)).sum().backward()
            opt.step()
        _ref_step(algo, W, states, ids, coef, t)
        assert np.array_equal(_bits(embs[0].weight), _bits(embs[1].weight))
        assert np.array_equal(_bits(embs[0].weight), W.view(np.uint32))


def test_two_tables_under_one_optimizer_and_a_settable_lr(thg):
    rng = np.random.default_rng(77)
    a, b = thg.SparseEmbedding(V, D, seed=1), thg.SparseEmbedding(V, D, seed=2)
    opt = thg.SparseSGD([a, b], lr=LR)
    Wa, Wb = a.weight.cpu().numpy().copy(), b.weight.cpu().numpy().copy()
    ids, coef = rng.integers(0, V, 8).astype(np.int64), _grad(rng, (8, D))
    (a(_cuda(ids)) * _cuda(coef)).sum().backward()   # b is not used in this step: it stays as it is
    opt.lr = 0.5
    opt.step()
    u, g, _ = eref.coalesce(ids, coef, V)
    eref.update(eref.SGD, Wa, u, g, alpha=0.5)
    assert np.array_equal(_bits(a.weight), Wa.view(np.uint32)) and np.array_equal(_bits(b.weight), Wb.view(np.uint32))
    (b(_cuda(ids)) * _cuda(coef)).sum().backward()
    opt.zero_grad()  # drops it
    opt.step()
    assert np.array_equal(_bits(b.weight), Wb.view(np.uint32))


@pytest.mark.parametrize("algo", [eref.ADAGRAD, eref.ADAM])
def test_state_dict_round_trip_continues_with_the_same_bits(thg, algo):
    rng = np.random.default_rng(algo)
    emb = thg.SparseEmbedding(V, D, seed=5)
    opt = _make(thg, algo, emb)
    batches = [(rng.integers(0, V, 10).astype(np.int64), _grad(rng, (10, D))) for _ in range(3)]

    def step(e, o, batch):
        (e(_cuda(batch[0])) * _cuda(batch[1])).sum().backward()
        o.step()

    for batch in batches[:2]:
        step(emb, opt, batch)
    sd_emb, sd_opt = copy.deepcopy(emb.state_dict()), copy.deepcopy(opt.state_dict())
    assert sd_opt["state"][0]["step"] == 2 and sd_opt["state"][0]["state1"] is not None
    emb2 = thg.SparseEmbedding(V, D, seed=6)
    emb2.load_state_dict(sd_emb)
    opt2 = _make(thg, algo, emb2)
    opt2.load_state_dict(sd_opt)
    step(emb, opt, batches[2])
    step(emb2, opt2, batches[2])
    assert np.array_equal(_bits(emb.weight), _bits(emb2.weight))
    for key in ("state1", "state2"):
        if opt.state[0][key] is not None:
            assert np.array_equal(_bits(opt.state[0][key]), _bits(opt2.state[0][key]))
            assert opt2.state[0][key].data_ptr() != sd_opt["state"][0][key].data_ptr()  # a copy, not the dict's tensor
    assert opt2.state[0]["step"] == 3


def test_value_errors(thg):
    import torch
    emb = thg.SparseEmbedding(V, D)
    with pytest.raises(ValueError, match="int64"):
        emb(torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="ids live on"):
        emb(torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="torch tensor"):
        emb([0, 1])
    with pytest.raises(ValueError, match="dim"):
        thg.SparseEmbedding(4, 2 ** 31)
    with pytest.raises(ValueError, match="dim"):
        thg.SparseEmbedding(4, 0)
    with pytest.raises(ValueError, match="num_rows"):
        thg.SparseEmbedding(2 ** 31 - 1, 4)
    wide = thg.SparseEmbedding(1, 2 ** 20)
    with pytest.raises(ValueError, match="n \\* dim exceeds int32"):
        wide(torch.zeros(2 ** 11, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="SparseEmbedding modules"):
        thg.SparseSGD([torch.nn.Linear(2, 2)], lr=0.1)
    out = emb(torch.tensor([1, 2], device="cuda"))
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(out.sum(), [emb._anchor], create_graph=True)


def test_example_trains_and_repeats_its_losses():
    """examples/train_node2vec.py, one short epoch twice from one seed in a process of its own: the loss falls inside the
    epoch and the two runs print the same 16 per-batch losses bit for bit"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_node2vec.py"), "1", "4096"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("run ")]
    assert len(lines) == 2, r.stdout[-2000:]
    first, second = (float(v) for v in lines[0].split("loss ")[1].split(" (")[0].split(" -> "))
    assert second < first, lines[0]
    bits = [ln.split("bits ")[1] for ln in lines]
    assert bits[0] == bits[1] and len(bits[0].split(",")) == 16, lines
    assert "the two runs' losses are the same bits" in r.stdout
