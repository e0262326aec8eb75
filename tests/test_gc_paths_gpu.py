"""k_gc's two scratch tiers (a collection's working arrays in LDS, or in the global scratch
alone for trees past the LDS budget) and its dynamic queue: a collection is invisible to the
search, so every run stays bit-exact with the oracle whichever tier collected a tree and
however the queue's entries were shared out. spl_diag_gc_paths says which way the
collections went; spl_diag_gc_lds_limit moves the tier boundary so that small trees drive
both tiers."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _oracle as O  # noqa: E402
from test_mcts_gpu import mcts_for  # noqa: E402
from test_selfplay_gpu import HDR_KEYS, _deep_device, _oracle_lagged, sort_examples  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 64, 3000), (4, 32, 2000)]      # players, games, iterations (100 simulations, genbu)
SEED = 11


def _lib():
    from splendor import _lib as lib
    L = lib.lib()
    L.spl_diag_gc_paths.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.spl_diag_gc_paths.restype = ctypes.c_int
    L.spl_diag_gc_lds_limit.argtypes = [ctypes.c_int]
    L.spl_diag_gc_lds_limit.restype = ctypes.c_int
    return L


def gc_paths(reset=False):
    """(LDS collections, fallback collections, most queue entries of one workgroup, launches
    with work)"""
    torch.cuda.synchronize()
    out = (ctypes.c_ulonglong * 4)()
    assert _lib().spl_diag_gc_paths(out, 1 if reset else 0) == 0
    return tuple(int(x) for x in out)


@pytest.fixture(autouse=True)
def gc_diag():
    L = _lib()
    gc_paths(reset=True)
    L.spl_diag_gc_lds_limit(-1)
    yield L
    gc_paths(reset=True)
    L.spl_diag_gc_lds_limit(-1)


_refs = {}


def _reference(n, B, iters, lag):
    """the oracle's run of a shape, computed once and shared (read-only) by the tiers' tests"""
    key = (n, B, iters, np.asarray(lag).tobytes())
    if key not in _refs:
        _refs[key] = _oracle_lagged(n, B, iters, SEED, 100, lag)
    return _refs[key]


def _check_against_oracle(n, B, iters, run):
    hdr, st, ex = run
    ref = _reference(n, B, iters, hdr["withdrawals"])
    rh = ref["hdr"]
    for k, j in (("player", 0), ("episode_step", 1), ("move_no", 2), ("game_no", 3), ("games_done", 4),
                 ("moves", 5), ("sims_done", 6)):
        np.testing.assert_array_equal(hdr[k], rh[:, j], err_msg=k)
    dsum, dmax, _ = ref["depth"]
    assert st["depth_sum"] == dsum and st["depth_max_all"] == dmax     # every simulation's leaf depth
    assert len(ex["pi"]) == len(ref["pi"])
    if len(ex["pi"]):
        ex = sort_examples(ex, ex["meta"])
        rf = sort_examples(ref, ref["meta"])
        for k, rk in (("meta", "meta"), ("board", "ex_board"), ("pi", "pi"), ("winner", "winner"),
                      ("scdiff", "scdiff"), ("surprise", "surprise")):
            np.testing.assert_array_equal(ex[k], rf[rk], err_msg=k)
        np.testing.assert_array_equal(ex["valids"].view(np.uint64), rf["valids"])
    assert st["prunes"] == st["resets"] == st["unexpanded"] == 0


@pytest.mark.parametrize("n,B,iters", SHAPES)
def test_lds_tier_matches_oracle(n, B, iters):
    run = _deep_device(n, B, iters, seed=SEED)
    lds, fallback, _, launches = gc_paths()
    print(f"gc paths n={n}: lds {lds} fallback {fallback} launches {launches}", flush=True)
    _check_against_oracle(n, B, iters, run)
    assert lds > 0 and fallback == 0 and launches > 0


@pytest.mark.parametrize("n,B,iters", SHAPES)
def test_fallback_tier_matches_oracle(gc_diag, n, B, iters):
    gc_diag.spl_diag_gc_lds_limit(0)
    run = _deep_device(n, B, iters, seed=SEED)
    lds, fallback, _, launches = gc_paths()
    print(f"gc paths n={n}, limit 0: lds {lds} fallback {fallback} launches {launches}", flush=True)
    _check_against_oracle(n, B, iters, run)
    assert fallback > 0 and lds == 0 and launches > 0


def test_mixed_tiers_match_oracle(gc_diag):
    """The tier boundary at 600 nodes: between the live-node median and the node counts before
    a collection of these trees, so one run takes both tiers."""
    n, B, iters = SHAPES[0]
    assert gc_diag.spl_diag_gc_lds_limit(600) == -1
    run = _deep_device(n, B, iters, seed=SEED)
    lds, fallback, _, _ = gc_paths()
    print(f"gc paths, limit 600: lds {lds} fallback {fallback}", flush=True)
    _check_against_oracle(n, B, iters, run)
    assert lds > 0 and fallback > 0


_search_ref = {}


def _oracle_searches(e, n, B, sims, seed, moves):
    """the oracle's side of `moves` searches with tree reuse and argmax play from the dealt
    boards: per move the visit counts and the boards after the move; computed once, shared
    (read-only) by both tiers' runs"""
    key = (n, B, sims, seed, moves)
    if key in _search_ref:
        return _search_ref[key]
    st = e.new_state(B)
    player = torch.zeros(B, dtype=torch.int8, device="cuda")
    e.init(st, player, seed=seed, stream=0xFFFFFFFF)
    oracles = [O.Mcts(n, sims, 1.5, 0.2, False) for _ in range(B)]
    host = st.cpu().numpy().copy()
    hp = np.zeros(B, np.int64)
    counts, boards = [], []
    for mv in range(moves):
        cm = []
        for b in range(B):
            c = host[b] if hp[b] == 0 else O.swap_players(n, host[b], int(hp[b]))
            oc, _, _, _, _ = oracles[b].search(c)
            cm.append(np.asarray(oc).copy())
            u = [O.uniform(seed, b, 1000 + mv, k) for k in range(2)]
            host[b], hp[b], _ = O.make_move(n, host[b], int(cm[-1].argmax()), int(hp[b]), False, u)
        counts.append(np.stack(cm))
        boards.append(host.copy())
    _search_ref[key] = (counts, boards)
    return _search_ref[key]


@pytest.mark.parametrize("limit", (-1, 0))
def test_more_queue_entries_than_workgroups(gc_diag, limit):
    """Search-only arenas collect every tree at every search start: 1,024 queue entries per
    launch for 256 workgroups, on either tier. Six searches with tree reuse, argmax play,
    against the oracle's searches."""
    from splendor.env import SplendorEngine
    gc_diag.spl_diag_gc_lds_limit(limit)
    n, B, sims, seed, moves = 2, 1024, 16, 77, 6
    e = SplendorEngine(n)
    ref_counts, ref_boards = _oracle_searches(e, n, B, sims, seed, moves)
    m = mcts_for(e, B, sims, 1.5, 0.2, False)
    st = e.new_state(B)
    player = torch.zeros(B, dtype=torch.int8, device="cuda")
    e.init(st, player, seed=seed, stream=0xFFFFFFFF)
    gc_paths(reset=True)
    for mv in range(moves):
        canon = e.canonical(st, player)
        _, _, _, counts = m.get_action_prob(canon, force_full_search=True, keep_tree=True)
        counts = counts.cpu().numpy()
        hdr = m.headers()
        assert hdr["overflow"].max() == 0
        np.testing.assert_array_equal(counts, ref_counts[mv], err_msg=f"move {mv}")
        action = counts.argmax(1)
        nxt = torch.empty(B, dtype=torch.int8, device="cuda")
        e.step(st, torch.from_numpy(action.astype(np.int16)).cuda(), player, nxt, deterministic=False,
               seed=seed, stream=1000 + mv)
        player = nxt
        np.testing.assert_array_equal(st.cpu().numpy(), ref_boards[mv])
    assert hdr["prunes"].sum() == hdr["resets"].sum() == hdr["unexpanded"].sum() == 0
    lds, fallback, most, launches = gc_paths()
    print(f"gc paths B={B}, limit {limit}: lds {lds} fallback {fallback} most {most} launches {launches}", flush=True)
    assert most >= 2
    assert (fallback > 0 and lds == 0) if limit == 0 else (lds > 0 and fallback == 0)


def _pressure_run():
    """tools/chk_pressure.py's shape at B = 64: per-tree maxima so small that search starts do
    not fit after a plain compaction, so k_gc prunes (compact_tree's second, linked pass)"""
    from splendor.env import SplendorEngine
    from splendor.mcts import HashEvaluator
    from splendor.selfplay import SelfPlay
    genbu = dict(cpuct=2.5, fpu=0.3, prob_fullMCTS=0.25, ratio_fullMCTS=5, forced_playouts=False,
                 dirichletAlpha=0.3, temperature=[1.25, 0.8], tempThreshold=10)
    e = SplendorEngine(2)
    sp = SelfPlay(e, 64, dict(genbu, numMCTSSims=64), evaluator=HashEvaluator(e), dirichlet_noise=True,
                  seed=0x5EED, node_cap=96, edge_cap=96 * 24)
    sp.reset()
    sp.run(800, use_graph=True)
    torch.cuda.synchronize()
    hdr, st = sp.headers(), sp.stats()
    ex = {k: v.cpu().numpy() for k, v in sp.drain().items()}
    return hdr, st, ex


def test_prune_pass_in_lds_equals_fallback(gc_diag):
    """Both passes of a pruning collection in LDS against the same run on the fallback tier
    (the global scratch alone), array for array."""
    a = _pressure_run()
    lds, fallback, _, _ = gc_paths(reset=True)
    assert lds > 0 and fallback == 0
    gc_diag.spl_diag_gc_lds_limit(0)
    b = _pressure_run()
    lds, fallback, _, _ = gc_paths()
    assert fallback > 0 and lds == 0
    print(f"pressure: {a[1]}", flush=True)
    assert a[1]["prunes"] > 0
    assert a[1] == b[1]
    # (every header field but the root's global node id, which follows the shared pools' pages)
    for k in [k for k in HDR_KEYS if k != "root"] + ["withdrawals", "gcs", "prunes", "resets", "unexpanded",
                                                      "depth_sum", "depth_max"]:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    ea, eb = sort_examples(a[2], a[2]["meta"]), sort_examples(b[2], b[2]["meta"])
    assert ea.keys() == eb.keys() and len(a[2]["meta"]) == len(b[2]["meta"])
    for k in ea:
        np.testing.assert_array_equal(ea[k], eb[k], err_msg=k)
