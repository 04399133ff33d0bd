"""Destination lists for kernels.edges_by_destination and a plain-loop check of the plan it returns, shared by
test_scatter_plan_host.py (the plan on CPU tensors) and test_gpu_point_index.py (hvpr_segment_sum_rows_f32 over the same plans)."""
import numpy as np

CHUNK = 32                                                        # kernels._SEG_CHUNK, restated: the tests pin the value
FANINS = (0, 1, 31, 32, 33, 63, 64, 65, 2000, 0, 0, 5)          # edges per destination; 2000 -> 63 chunks, two empty between full ones


def dst_of_fanins(fanins, seed):
    """int64 (E,): destination d appears fanins[d] times, in a seeded shuffle."""
    dst = np.repeat(np.arange(len(fanins), dtype=np.int64), np.asarray(fanins, np.int64))
    return np.random.default_rng(seed).permutation(dst)


def with_out_of_range(dst, n_dst, seed, n_bad=300):
    """dst with n_bad ids outside [0, n_dst) mixed in at random places: -1, a very negative one, n_dst, far past n_dst."""
    rng = np.random.default_rng(seed)
    bad = rng.choice(np.array([-1, -(2 ** 40), -7, n_dst, n_dst + 1, 2 ** 40], np.int64), n_bad)
    out = np.concatenate([dst, bad])
    return out[rng.permutation(len(out))]


def cases():
    """name -> (dst int64 (E,), n_dst)."""
    n = len(FANINS)
    base = dst_of_fanins(FANINS, 1)
    return {
        "fanins": (base, n),
        "fanins_with_dropped": (with_out_of_range(base, n, 2), n),
        "all_dropped": (with_out_of_range(np.zeros(0, np.int64), n, 3, n_bad=77), n),
        "no_edges": (np.zeros(0, np.int64), n),
        "n_dst_far_above_E": (np.random.default_rng(4).integers(0, 5000, 40).astype(np.int64), 5000),
        "one_destination_2000": (np.zeros(2000, np.int64), 1),
    }


def check_plan(dst, n_dst, order, chunk_ptr, dest_ptr):
    """The invariants of (order, chunk_ptr, dest_ptr), checked by a loop over destinations and chunks; all arguments are numpy
    arrays / ints.  Returns the number of chunks in use."""
    dst = np.asarray(dst).reshape(-1)
    E = len(dst)
    # lengths: the chunk count is bounded by E // CHUNK + min(n_dst, E); chunk_ptr keeps one spare chunk beyond the bound
    n_max = E // CHUNK + min(n_dst, E) + 1
    assert len(order) == E and len(chunk_ptr) == n_max + 1 and len(dest_ptr) == n_dst + 1
    assert sorted(order.tolist()) == list(range(E)), "order is not a permutation of the edge ids"
    assert dest_ptr[0] == 0 and (np.diff(dest_ptr) >= 0).all() and (np.diff(chunk_ptr) >= 0).all()
    assert chunk_ptr.min() >= 0 and chunk_ptr.max() <= E
    used = int(dest_ptr[n_dst])
    assert used <= E // CHUNK + min(n_dst, E)
    for d in range(n_dst):
        want = np.nonzero(dst == d)[0].tolist()                    # ascending edge ids
        got = []
        for c in range(int(dest_ptr[d]), int(dest_ptr[d + 1])):
            piece = order[int(chunk_ptr[c]):int(chunk_ptr[c + 1])].tolist()
            assert 1 <= len(piece) <= CHUNK, f"destination {d}: chunk {c} has {len(piece)} edges"
            got += piece
        assert got == want, f"destination {d} (fan-in {len(want)}): edges {got[:8]}... != {want[:8]}..."
        assert int(dest_ptr[d + 1]) - int(dest_ptr[d]) == -(-len(want) // CHUNK), f"destination {d}: chunk count"
    for c in range(used, n_max):
        assert chunk_ptr[c] == chunk_ptr[c + 1], f"chunk {c} past the last used one ({used}) is not empty"
    return used
