"""What tests/test_instances_gpu.py rests on, checked without a GPU: every entry of the instance matrix (tests/instance_cases.py) has
oracle chains, cold and continued, whose every decision is clear of a tie — |chi²_step - chi²_best| / chi²_best >= 1e-9 at every step
(test_sets_host.MARGIN), for Kholodenko >= 1e-5 at chi² >= 1 (test_sets_host.KHOLODENKO_MARGIN, where that derivation holds) — that
move at least three times and fewer than the trace holds, differently in the two repetitions, and differently cold and continued.
Then "the device takes the oracle's decisions" is a fair demand of every instance.  Kholodenko's chains are recorded
(tests/golden/instance_chains_kholodenko.npz, oracle/make_instance_chains.py): the recording belongs to the inputs as
instance_cases builds them now, and its two smallest shapes are computed again."""
import numpy as np
import pytest

from oracle import mcsas_oracle as O
import instance_cases as IC
from test_sets_host import KHOLODENKO_MARGIN, MARGIN


def test_the_matrix_is_the_lookup_tables():
    """8 models x (1, 2, 4, 8, 16 slots with and without cached rows, 32 and 64 with) = 96 wave tests of six forms; 8 models x (8, 16,
    32 slots) = 24 q-split instances of four forms in 45 tests; the shapes' last slots hold real points and padding."""
    assert len(IC.WAVE) == 96 and len(set(IC.WAVE)) == 96 and len(IC.WAVE) * 6 == 576
    assert len(IC.WIDE) == 45 and len({(t, q) for t, q, _ in IC.WIDE}) * 4 == 96
    assert [IC.wave_nq(q) for q in IC.WAVE_QPL] == [37, 101, 229, 485, 997, 2021, 4069]
    assert {(tag, qpl) for tag, qpl, cache in IC.WAVE if cache == 0} == {(tag, qpl) for tag in IC.MODELS for qpl in (1, 2, 4, 8, 16)}
    for qpl, shapes in IC.WIDE_SHAPES.items():
        (a, wa), (b, wb) = shapes["A"], shapes["B"]
        per_wave = 64 * qpl
        assert a == (wa - 1) * per_wave + 1 and wb == 8 and b == 7 * per_wave + 64 * (qpl - 1) + 37
        assert a > 8 * 64 * (qpl // 2) or qpl == 8                          # (too many points for the next smaller slot count)
    assert [(q, s) for t, q, s in IC.WIDE if t == "kholodenko"] == [(8, "A"), (16, "A"), (32, "A")]
    assert len(IC.ENTRIES) == 7 * 12 + 10 and len(IC.KHOLODENKO_NQ) == 10 and IC.REP_OFFSET > 0 and IC.R == 2
    for tag, nq in IC.ENTRIES:
        n, steps = IC.budget(tag, nq)
        assert (n, steps) == (12, 64) if tag != "kholodenko" else (n == 6 and 16 <= steps <= 24)
        assert steps < IC.CAPACITY
        cold, cont = IC.seeds(tag, nq)
        assert cold != cont                                                   # the continued chain runs on a stream of its own


@pytest.mark.parametrize("tag,nq", IC.ENTRIES)
def test_every_chain_of_the_matrix_is_decisive_and_moves(tag, nq):
    both = IC.chains(tag, nq)
    n, steps = IC.budget(tag, nq)
    bound = KHOLODENKO_MARGIN if tag == "kholodenko" else MARGIN
    for kind in ("cold", "cont"):
        for r, c in enumerate(both[kind]):
            ref = c["ref"]
            print(tag, nq, kind, "rep", r, "min margin %.3e" % c["margin"], "steps", ref.num_iter, "moves", ref.num_moves,
                  "lowest chi2 %.6g" % c["lowest"])
            assert c["attempts"] == 1 and c["converged"] == 0 and ref.num_iter == steps          # to the budget
            assert c["margin"] >= bound
            assert IC.MIN_MOVES <= ref.num_moves < IC.CAPACITY
            if tag == "kholodenko":
                assert c["lowest"] >= 1.0
            P = ref.rset.shape[1]
            assert c["pos"][-1] == P * steps + (0 if kind == "cont" else P * n)               # no draws for a given set
        a, b = both[kind]
        assert not np.array_equal(a["trace"]["step"], b["trace"]["step"])                      # the repetitions differ in their moves
        assert not np.array_equal(a["ref"].rset, b["ref"].rset)
    for r in range(IC.R):
        cold, cont = both["cold"][r], both["cont"][r]
        assert not np.array_equal(cold["ref"].rset, cont["ref"].rset)
        assert not np.array_equal(cold["trace"]["values"][:3], cont["trace"]["values"][:3])    # (a stream of its own)
        np.testing.assert_allclose(cont["trace"]["chisq0"], cold["ref"].conval, rtol=1e-9)      # it starts where the cold one ended
    start = IC.start_array(both)
    assert start.shape == (n, both["cold"][0]["ref"].rset.shape[1], IC.R + 2)
    assert np.isnan(start[:, :, 0]).all() and np.isnan(start[:, :, IC.R + 1]).all() and np.isfinite(start[:, :, 1:IC.R + 1]).all()
    for r in range(IC.R):
        assert np.array_equal(start[:, :, 1 + r], both["cold"][r]["ref"].rset)


def test_the_recording_belongs_to_the_inputs_of_today():
    g = IC.fixture()
    assert sorted(set(int(n) for n in g["index"][:, 0])) == sorted(IC.KHOLODENKO_NQ) and len(g["index"]) == 4 * len(IC.KHOLODENKO_NQ)
    assert all(a.dtype.kind in "iuf" for a in g.values())                                      # numbers only
    for nq in IC.KHOLODENKO_NQ:
        both = IC.chains("kholodenko", nq)
        s_cold, s_cont = IC.seeds("kholodenko", nq)
        for r in range(IC.R):
            assert np.array_equal(both["cold"][r]["digest"], IC.digest("kholodenko", nq, r, None, s_cold)), (nq, r)
            assert np.array_equal(both["cont"][r]["digest"], IC.digest("kholodenko", nq, r, both["cold"][r]["ref"].rset, s_cont)), (nq, r)


@pytest.mark.parametrize("nq", [37, 101])
def test_the_recording_is_what_the_oracle_computes(nq):
    """The two smallest shapes again, in this process: every stored number bit for bit."""
    now, then = IC.compute_chains("kholodenko", nq), IC.chains("kholodenko", nq)
    for kind in ("cold", "cont"):
        for a, b in zip(now[kind], then[kind]):
            ra, rb = a["ref"], b["ref"]
            assert (ra.num_iter, ra.num_moves, a["pos"], a["attempts"], a["converged"]) == (rb.num_iter, rb.num_moves, b["pos"], 1, 0)
            assert np.array_equal(ra.rset, rb.rset)
            assert (ra.conval, ra.scaling, ra.background, a["margin"], a["lowest"]) == (rb.conval, rb.scaling, rb.background, b["margin"], b["lowest"])
            for f in ("chisq0", "step", "chisq", "values"):
                assert np.array_equal(a["trace"][f], b["trace"][f]), f
    q, I, sig = IC.data(nq)
    _, spec = IC.models("kholodenko")
    assert isinstance(spec, O.ModelSpec) and spec.n_active == 3 and len(q) == nq
