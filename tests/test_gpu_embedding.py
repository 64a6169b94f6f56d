"""glx_rows_coalesce and glx_embedding_update on the GPU against the numpy restatement of the contracts
(embedding_ref.py), at tolerance 0: bit equality, the sign of zero included.  Every output buffer starts as a canary (NaN
gradients, -7 rows), so what a call must not write is seen untouched."""
import numpy as np
import pytest

import embedding_ref as eref
import glx

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
CANARY_ROW = -7
# the kernels' own launch constants (glx_embedding.hip): workgroups of 256 lanes, lane groups of 8 .. 64 lanes -- one
# group per sorted position (reduce) or per window of COALESCE_CHUNK + 1 sorted positions (combine), per entry (update)
WORKGROUP = 256
SMALLEST_GROUP, LARGEST_GROUP = 8, 64
DIM_OF_GROUP = {SMALLEST_GROUP: 4, LARGEST_GROUP: 256}  # dim / 4 lanes: 1 -> a group of 8; 64 -> a group of 64
WINDOW = glx.COALESCE_CHUNK + 1


def _cuda(a, offset=False):
    """a CUDA copy of `a`; offset: 4 bytes into its buffer, so that it is not 16-byte aligned"""
    import torch
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).cuda()
    assert a.dtype == np.float32
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _mixed(rng, shape):
    """float32 values over seven decades: the order of a sum shows in its bits"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


def gpu_coalesce(rows, g, num_rows, host=False, offset=False):
    """(urows, ug, count) as numpy / int from one call whose outputs start as canaries"""
    n, D = g.shape
    urows, ug = np.full(n, CANARY_ROW, np.int64), np.full((n, D), NAN, np.float32)
    if host:
        _, _, count = glx.rows_coalesce(rows, g, num_rows, out_rows=urows, out_g=ug)
        return urows, ug, count
    d_urows, d_ug = _cuda(urows), _cuda(ug)
    _, _, count = glx.rows_coalesce(_cuda(rows), _cuda(g, offset), num_rows, out_rows=d_urows, out_g=d_ug)
    assert count.is_cuda and count.numel() == 1  # no host read inside the call
    return d_urows.cpu().numpy(), d_ug.cpu().numpy(), int(count.cpu()[0])


def check_coalesce(rows, g, num_rows, offset=False, host=True):
    """device pointers twice, host pointers once, against the restatement"""
    assert not np.isnan(g).any()
    want_urows, want_ug, U = eref.coalesce(rows, g, num_rows)
    runs = [gpu_coalesce(rows, g, num_rows, offset=offset) for _ in range(2)]
    if host:
        runs.append(gpu_coalesce(rows, g, num_rows, host=True))
    for urows, ug, count in runs:
        assert count == U
        assert np.array_equal(urows, want_urows), "urows: the distinct rows ascending, then -1"
        assert eref.same_bits(ug[:U], want_ug)
        assert np.array_equal(ug[:U].view(np.uint32), want_ug.view(np.uint32))
        assert np.isnan(ug[U:]).all(), "a row of ug past U was written"
    return runs[0]


DIMS = (1, 3, 4, 20, 64, 100, 256, 260)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dim", DIMS)
def test_every_dimension_path(dim, offset):
    """VEC 4 and 1, every group size, more columns than one tile (260, 100 scalar); rows with -1 and num_rows among them;
    lists of at most 256 positions: also glx_aggregate_backward's Sum rows, bit for bit"""
    rng = np.random.default_rng(dim)
    V, n = 23, 90
    rows = rng.integers(-1, V + 1, n).astype(np.int64)
    rows[0], rows[1], rows[2] = -1, V, 5
    g = _mixed(rng, (n, dim))
    g[2, 0] = -0.0
    urows, ug, U = check_coalesce(rows, g, V, offset=offset)
    dense = glx.aggregate_backward(glx.SUM, _cuda(rows), None, _cuda(g), V).cpu().numpy()
    assert eref.same_bits(ug[:U], dense[urows[:U]])
    untouched = np.setdiff1d(np.arange(V), urows[:U])
    assert not dense[untouched].any()


@pytest.mark.parametrize("dim", [4, 20])
@pytest.mark.parametrize("times", [1, 255, 256, 257, 512, 513, 1025])
def test_one_row_repeated_around_the_chunk_size(times, dim):
    """one row `times` times among others that occur once, its positions scattered: one chunk, exactly one, one entry
    past it, two, two and one entry, four and one entry"""
    rng = np.random.default_rng(times + dim)
    V = 40
    rows = np.concatenate([np.full(times, 17), np.delete(np.arange(V), 17)[:12]]).astype(np.int64)
    rng.shuffle(rows)
    g = _mixed(rng, (len(rows), dim))
    urows, ug, U = check_coalesce(rows, g, V, host=times in (257, 1025))
    assert U == 13
    if times <= glx.COALESCE_CHUNK:
        dense = glx.aggregate_backward(glx.SUM, _cuda(rows), None, _cuda(g), V).cpu().numpy()
        assert eref.same_bits(ug[:U], dense[urows[:U]])


def test_the_chunk_rule_on_the_device():
    """256 ones then three times 2^-17 on one row: 256 + 2^-15 under the contract, 256 in plain ascending order"""
    rows = np.zeros(259, np.int64)
    g = np.concatenate([np.ones(256, np.float32), np.full(3, 2.0 ** -17, np.float32)])[:, None].repeat(4, 1)
    _, ug, U = check_coalesce(rows, np.ascontiguousarray(g), 1)
    assert U == 1 and np.all(ug[0] == np.float32(256 + 2.0 ** -15))


def test_empty_and_all_dropped_requests():
    """n = 0 writes the count alone; a request whose rows are all outside the table writes the -1 fill and a count of 0"""
    import torch
    for host in (False, True):
        urows, ug, count = gpu_coalesce(np.zeros(0, np.int64), np.zeros((0, 8), np.float32), 5, host=host)
        assert count == 0 and urows.shape == (0,) and ug.shape == (0, 8)
        rows = np.array([-1, 5, 6, -(2 ** 40), 2 ** 40], np.int64)
        urows, ug, count = gpu_coalesce(rows, np.ones((5, 8), np.float32), 5, host=host)
        assert count == 0 and urows.tolist() == [-1] * 5 and np.isnan(ug).all()
    # a table of no rows drops everything as well
    urows, ug, count = gpu_coalesce(np.array([0, 1], np.int64), np.ones((2, 4), np.float32), 0)
    assert count == 0 and urows.tolist() == [-1, -1] and np.isnan(ug).all()
    torch.cuda.synchronize()


def test_rows_up_to_the_sort_s_top_bit():
    """num_rows = 2^31 - 2 with no table behind it: nothing is allocated or launched per row of the table"""
    num_rows = 2 ** 31 - 2
    rows = np.array([num_rows - 1, 0, 2 ** 30, num_rows, -1, 2 ** 30, num_rows - 1, 0, 2 ** 31 - 1, 2 ** 32], np.int64)
    g = _mixed(np.random.default_rng(8), (len(rows), 4))
    urows, ug, U = check_coalesce(rows, g, num_rows)
    assert urows[:U].tolist() == [0, 2 ** 30, num_rows - 1]


@pytest.mark.parametrize("group", [SMALLEST_GROUP, LARGEST_GROUP])
@pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_group_short", "exactly_one_workgroup", "one_group_more"])
def test_position_counts_at_the_reduce_kernel_s_workgroup_edges(edge, group):
    """the reduce kernel: one group per sorted position, WORKGROUP / group positions per workgroup"""
    dim, n = DIM_OF_GROUP[group], WORKGROUP // group + edge
    rng = np.random.default_rng(n)
    rows = rng.integers(-1, n + 1, n).astype(np.int64)
    check_coalesce(rows, _mixed(rng, (n, dim)), n)


@pytest.mark.parametrize("n", [WORKGROUP - 1, WORKGROUP, WORKGROUP + 1])
def test_position_counts_at_the_key_and_flag_kernels_workgroup_edges(n):
    """the key and flag kernels: one lane per position, WORKGROUP positions per workgroup; one row fills a whole chunk
    and, at WORKGROUP + 1 positions, starts a second"""
    rng = np.random.default_rng(n)
    check_coalesce(np.full(n, 2, np.int64), _mixed(rng, (n, 4)), 3, host=False)
    check_coalesce(rng.integers(-1, 9, n).astype(np.int64), _mixed(rng, (n, 3)), 8, host=False)


@pytest.mark.parametrize("group", [SMALLEST_GROUP, LARGEST_GROUP])
@pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_group_short", "exactly_one_workgroup", "one_group_more"])
def test_position_counts_at_the_combine_kernel_s_workgroup_edges(edge, group):
    """the combine kernel: one group per window of WINDOW sorted positions, WORKGROUP / group windows per workgroup.  n
    ends one window short of a workgroup, fills it, and goes one position into the next; two rows of more than one chunk,
    one whose head lies in the last window that can hold one"""
    dim = DIM_OF_GROUP[group]
    windows = WORKGROUP // group
    n = WINDOW * (windows - 1) if edge < 0 else WINDOW * windows + (1 if edge > 0 else 0)
    rng = np.random.default_rng(n + dim)
    V = 60
    long_a, long_b = WINDOW + 1, WINDOW  # rows 0 and V - 1: two chunks each, the second of one and of two entries
    rows = np.concatenate([np.zeros(long_a), np.full(long_b, V - 1), rng.integers(1, V - 1, n - long_a - long_b)])
    rows = rows.astype(np.int64)
    rng.shuffle(rows)
    g = _mixed(rng, (n, dim))
    urows, ug, U = check_coalesce(rows, g, V, host=False)
    assert urows[0] == 0 and urows[U - 1] == V - 1  # sorted, row V - 1's head is position n - WINDOW: the last window's first


# ---- the optimizer steps ------------------------------------------------------------------------------------------
ALGOS = [eref.SGD, eref.ADAGRAD, eref.ADAM]


def _magnitudes(rng, shape):
    """signed float32 values with magnitudes in [2^-10, 2^3]: no intermediate of a step is subnormal"""
    mag = np.exp2(rng.uniform(-10.0, 3.0, shape))
    return (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _scalars(algo, t):
    if algo == eref.ADAM:
        return eref.adam_scalars(0.01, (0.9, 0.999), 1e-8, t)
    return (0.05, 1e-10 if algo == eref.ADAGRAD else 0.0, 0.0, 0.0, 0.0, 0.0)


def _step_kw(sc):
    return dict(zip(("alpha", "eps", "beta1", "c1", "beta2", "c2"), sc))


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("dim", [1, 4, 20, 64, 260])
@pytest.mark.parametrize("algo", ALGOS)
def test_three_steps_leave_the_whole_table_as_the_restatement_does(algo, dim, offset):
    """the WHOLE table and the state tables after each of three steps, bit for bit: the rows a step names are updated
    with one rounding per operation, every other row is untouched; entries of -1 and num_rows are skipped"""
    rng = np.random.default_rng(100 * algo + dim)
    V, n = 37, 21
    W = _magnitudes(rng, (V, dim))
    states = [np.zeros((V, dim), np.float32) for _ in range({eref.SGD: 0, eref.ADAGRAD: 1}.get(algo, 2))]
    d_W = _cuda(W, offset)
    d_states = [_cuda(s, offset) for s in states] + [None, None]
    for t in range(1, 4):
        urows = rng.permutation(V)[:n].astype(np.int64)  # distinct
        urows[3], urows[7], urows[n - 1] = -1, V, -1
        ug = _magnitudes(rng, (n, dim))
        sc = _scalars(algo, t)
        eref.update(algo, W, urows, ug, *(states + [None, None])[:2], *sc)
        glx.embedding_update(algo, d_W, _cuda(urows), _cuda(ug, offset), state1=d_states[0], state2=d_states[1],
                             **_step_kw(sc))
        assert np.array_equal(d_W.cpu().numpy().view(np.uint32), W.view(np.uint32)), (algo, dim, t)
        for d_s, s in zip(d_states, states):
            assert np.array_equal(d_s.cpu().numpy().view(np.uint32), s.view(np.uint32)), (algo, dim, t)
    assert np.isfinite(W).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_a_step_over_no_entries_touches_nothing(algo):
    import torch
    W = _magnitudes(np.random.default_rng(2), (5, 8))
    d_W = _cuda(W)
    d_states = [_cuda(np.full((5, 8), 0.5, np.float32)) for _ in range({eref.SGD: 0, eref.ADAGRAD: 1}.get(algo, 2))]
    d_states += [None, None]
    empty_rows = torch.empty((0,), dtype=torch.int64, device="cuda")
    empty_g = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    glx.embedding_update(algo, d_W, empty_rows, empty_g, state1=d_states[0], state2=d_states[1],
                         **_step_kw(_scalars(algo, 1)))
    # and a step whose entries are all outside the table
    glx.embedding_update(algo, d_W, _cuda(np.array([-1, 5, -1], np.int64)), _cuda(np.ones((3, 8), np.float32)),
                         state1=d_states[0], state2=d_states[1], **_step_kw(_scalars(algo, 1)))
    assert np.array_equal(d_W.cpu().numpy().view(np.uint32), W.view(np.uint32))
    for s in d_states[:-2]:
        assert (s.cpu().numpy() == 0.5).all()


@pytest.mark.parametrize("group", [SMALLEST_GROUP, LARGEST_GROUP])
@pytest.mark.parametrize("edge", [-1, 0, 1], ids=["one_group_short", "exactly_one_workgroup", "one_group_more"])
def test_entry_counts_at_the_update_kernel_s_workgroup_edges(edge, group):
    """the update kernel: one group per entry, WORKGROUP / group entries per workgroup; Adam reads and writes the most"""
    dim, n = DIM_OF_GROUP[group], WORKGROUP // group + edge
    rng = np.random.default_rng(n + group)
    V = n + 5
    W, m, v = _magnitudes(rng, (V, dim)), np.zeros((V, dim), np.float32), np.zeros((V, dim), np.float32)
    urows, ug = rng.permutation(V)[:n].astype(np.int64), _magnitudes(rng, (n, dim))
    d_W, d_m, d_v = _cuda(W), _cuda(m), _cuda(v)
    sc = _scalars(eref.ADAM, 1)
    eref.update(eref.ADAM, W, urows, ug, m, v, *sc)
    glx.embedding_update(glx.EMB_ADAM, d_W, _cuda(urows), _cuda(ug), state1=d_m, state2=d_v, **_step_kw(sc))
    for got, want in ((d_W, W), (d_m, m), (d_v, v)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_coalesce_feeds_the_update_without_a_host_read():
    """the -1 tail of a coalesce and its unwritten gradient rows go straight into a step over n entries"""
    rng = np.random.default_rng(6)
    V, n, dim = 11, 40, 8
    rows = rng.integers(-1, V + 1, n).astype(np.int64)
    g, W = _magnitudes(rng, (n, dim)), _magnitudes(rng, (V, dim))
    d_W = _cuda(W)
    d_urows, d_ug, _ = glx.rows_coalesce(_cuda(rows), _cuda(g), V, out_g=_cuda(np.full((n, dim), NAN, np.float32)))
    glx.embedding_update(glx.EMB_SGD, d_W, d_urows, d_ug, alpha=0.05)
    urows, ug, U = eref.coalesce(rows, g, V)
    eref.update(eref.SGD, W, urows, ug, alpha=0.05)
    assert np.array_equal(d_W.cpu().numpy().view(np.uint32), W.view(np.uint32))


def test_bad_arguments_are_refused_on_the_device_too():
    import torch
    W = torch.zeros((4, 4), device="cuda")
    rows, g = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((2, 4), device="cuda")
    for call in (lambda: glx.embedding_update(7, W, rows, g, alpha=0.1),
                 lambda: glx.embedding_update(glx.EMB_ADAM, W, rows, g, state1=W.clone(), alpha=0.1),
                 lambda: glx.embedding_update(glx.EMB_SGD, W, rows, g, state1=W.clone(), alpha=0.1),
                 lambda: glx.rows_coalesce(rows, g, 2 ** 31 - 1)):
        with pytest.raises(glx.GlxError) as e:
            call()
        assert e.value.code == 3
