"""CPU side of the playout incumbents (rp_set_incumbent_playouts): the C ABI's declarations, and guards that the oracle-side reference of
tests/test_gpu_best_playout.py (tests/best_playout_ref.py) is not vacuous on the inputs that test plays."""
import functools
import os
import re

import best_playout_ref as bp
import best_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rp_set_incumbent_playouts", "rp_pop_finished_best_playouts", "rp_incumbent_sources", "rp_rollout_paths")


def test_header_library_and_bindings_declare_the_playout_abi():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == 10 == _lib.ABI_VERSION  # additive: the number stays
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    want = {"rp_set_incumbent_playouts": 2, "rp_pop_finished_best_playouts": 19, "rp_incumbent_sources": 5, "rp_rollout_paths": 9}
    for name in NEW:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]) == want[name], name
        assert hasattr(L, name), "librp_engine.so does not export " + name
    # rp_pop_finished_best's arguments plus the two sources
    assert len(_lib._SIGS["rp_pop_finished_best_playouts"][1]) == len(_lib._SIGS["rp_pop_finished_best"][1]) + 2
    for cite in ("MCTS_bpp.py:87", "BinPackingGame.py:58-76", "BinPackingGame.py:188-212"):
        assert text.count(cite) >= 5, cite  # each of the four new comments stands on them
    assert "8 (G + fin_cap) bytes" in text
    for method in ("set_incumbent_playouts", "incumbent_sources", "rollout_paths"):
        assert hasattr(_lib.Engine, method)


@functools.lru_cache(maxsize=None)
def probe_episodes():
    """The 32 episodes of the probe: best_ref.SHAPES, 3 playouts, the sampled rule, best_ref.BUF, seed 5, salt 9."""
    return [bp.probe(s, g)[1] for s, shape in enumerate(best_ref.SHAPES) for g in range(shape[5])]


def test_playouts_beat_the_tree_on_the_probe_shapes():
    """(a) some episode's incumbent with playouts scores strictly above its tree-only incumbent (21 of 32 when this was written), and
    none scores below it; the played packing is never better than either."""
    eps = probe_episodes()
    assert len(eps) == 32
    for r in eps:
        assert r["score"] >= r["tree"]["score"] >= r["played"]["score"]
        assert r["updates"] == len(r["sources"]) == len(r["history"]) and r["sources"][-1] == r["playout"]
        if r["playout"] >= 0:
            assert r["moves"] == r["tree_moves"] + len(r["actions"]) and r["prefix"] <= r["tree_moves"]
        else:
            assert r["moves"] == r["tree_moves"]
    better = sum(r["score"] > r["tree"]["score"] for r in eps)
    print("playout incumbent above the tree-only incumbent: %d of %d" % (better, len(eps)))
    assert better >= 1, "no playout beats its episode's tree: the GPU parity test would prove little"


def test_the_lowest_playout_among_equals_is_exercised():
    """(b) at least one winning leaf offer has several playouts sharing the maximum (11 when this was written): the offer is the first of
    them, which with 3 playouts is not the last."""
    tied = sum(r["tied_wins"] for r in probe_episodes())
    print("winning offers with a shared maximum: %d" % tied)
    assert tied >= 1, "the tie rule among playouts (lowest index) is never exercised"
    firsts = [h for r in probe_episodes() for h in r["history"] if h["tied"]]
    assert any(h["playout"] < bp.PLAYOUTS - 1 for h in firsts)


def test_a_tree_terminal_replaces_a_playout_incumbent_on_the_late_starts():
    """(c) never on the probe shapes, so it is pinned with the late-game starts: the instances best_playout_ref lists update P then T."""
    def t_after_p(sources):
        return any(a >= 0 and b == -1 for a, b in zip(sources, sources[1:]))

    assert not any(t_after_p(r["sources"]) for r in probe_episodes())
    inst = bp.late_instances()
    p_then_t = [k for k in range(bp.LATE_COUNT) if bp.late_episode(k, inst)["sources"] == [0, -1]]
    assert tuple(p_then_t) == bp.LATE_P_THEN_T and len(p_then_t) >= 1
    r = bp.late_episode(bp.LATE_P_THEN_T[0], inst)
    assert r["playout"] == -1 and r["tree_moves"] == r["moves"] == 1 and r["updates"] == 2 and r["history"][0]["playout"] == 0
