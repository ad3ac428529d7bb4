"""The q-split workgroup kernel (csrc/chain_wide.h: more than 1024 q-points, one workgroup per chain with the q-points split over
its waves) under the fit flags: find_background, positive_background, start_from_minimum, retries, and a convergence criterion
the chain reaches inside its budget.  The edge-shape and chain-end tests run this kernel with the default flags only.

Sphere, 16 contributions, 48 steps (three quarters of one 64-proposal block), 2 repetitions.
 * 1025 q-points: the first q-split shape (8 slots per lane, 3 waves, the last wave nearly all padding).  The wave-per-chain
   kernel still takes it, so the two kernels are compared with each other and both with the closed-form oracle.
 * 4097 q-points: the first 16-slot shape (5 waves), beyond the wave kernel: against the oracle only.
The oracle's side (which criterion converges, at least one accepted move per chain) is asserted on the oracle's own output and
runs without a device (test_oracle_side_of_every_case)."""
import functools
import itertools

import numpy as np
import pytest

from mcsas_amd import engine
from oracle import mcsas_oracle as O
from helpers import make_models, FakeData

N_CONTRIB, MAX_ITER, REPS, SEED = 16, 48, 2, 7
# Chi-squared of the oracle's chains on this data (both repetitions, every flag combination): 1700-9000 after the initial fit,
# 350-435 after 40 steps.  450 is below every start — so each chain needs an accepted move — and reached by step 40 of 48.
CONVERGING = 450.0
CASES_1025 = list(itertools.product((True, False), (False, True), (False, True), (0, 2), (1e-9, CONVERGING)))
CASES_4097 = list(itertools.product((True, False), (False, True)))


@functools.lru_cache(maxsize=None)
def _data(nq):
    from bench import synthetic_data
    q, I, sig = synthetic_data(nq)
    for v in (q, I, sig):
        v.setflags(write=False)
    return q, I, sig


def _models(q):
    return make_models("sphere", [np.pi / q.max()], [np.pi / q.min()])


@functools.lru_cache(maxsize=None)
def _oracle(nq, find_bg, pos_bg, from_min, retries, crit):
    """The oracle's chains: per repetition the attempts of McSAS.analyse (mcsas.py:220-246) on the repetition's own stream.
    -> list of (last attempt's ChainResult, attempts, draws)."""
    q, I, sig = _data(nq)
    _, spec = _models(q)
    ost = O.Settings(n_contrib=N_CONTRIB, n_reps=1, max_iter=MAX_ITER, conv_crit=crit, find_bg=find_bg, pos_bg=pos_bg,
                     start_from_min=from_min, max_retries=retries)
    out = []
    for r in range(REPS):
        stream = O.PhiloxStream(SEED, r)
        attempts = 0
        while True:
            ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, stream, method="closed")
            attempts += 1
            assert ref.num_moves >= 1, (nq, find_bg, pos_bg, from_min, retries, crit, r)     # a chain that decides something
            if not (ref.conval > crit) or attempts > retries:
                break
        if crit == CONVERGING:
            assert ref.conval <= crit and ref.num_iter < MAX_ITER and attempts == 1           # converges inside the budget
        else:
            assert ref.conval > crit and ref.num_iter == MAX_ITER and attempts == retries + 1
        out.append((ref, attempts, stream.pos))
    return out


def _run(nq, mode, find_bg, pos_bg, from_min, retries, crit):
    q, I, sig = _data(nq)
    m, _ = _models(q)
    st = engine.Settings(n_contrib=N_CONTRIB, n_reps=REPS, max_iter=MAX_ITER, conv_crit=crit, find_background=find_bg,
                         positive_background=pos_bg, start_from_minimum=from_min, max_retries=retries, seed=SEED, exec_mode=mode)
    setup = m.setup(FakeData(q))
    return engine.analyse(setup, q, I, sig, st), engine.Plan(setup, q, I, sig, st).info


def _check_against_oracle(res, refs, res_crit):
    for r, (ref, attempts, draws) in enumerate(refs):
        print("rep %d: chisq %.17g oracle %.17g, iter %d/%d moves %d/%d attempts %d/%d draws %d/%d" % (
            r, res.chisq[r], ref.conval, res.num_iter[r], ref.num_iter, res.num_moves[r], ref.num_moves, res.attempts[r], attempts,
            res.draws[r], draws))
        assert res.num_iter[r] == ref.num_iter and res.num_moves[r] == ref.num_moves
        assert res.attempts[r] == attempts and res.draws[r] == draws
        assert res.converged[r] == (0 if ref.conval > res_crit else 1)
        np.testing.assert_array_equal(res.contribs[:, :, r], ref.rset)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
        np.testing.assert_allclose(res.fit[:, r], ref.fit, rtol=1e-7)


def test_oracle_side_of_every_case():
    """No device: the oracle's chains of every case exist, accept at least one move each, and converge (or not) as the case says."""
    for c in CASES_1025:
        _oracle(1025, *c)
    for find_bg, pos_bg in CASES_4097:
        _oracle(4097, find_bg, pos_bg, False, 2, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("find_bg,pos_bg,from_min,retries,crit", CASES_1025)
def test_q_split_kernel_with_fit_flags_matches_wave_kernel_and_oracle(find_bg, pos_bg, from_min, retries, crit):
    refs = _oracle(1025, find_bg, pos_bg, from_min, retries, crit)
    wg, info = _run(1025, engine.EXEC_WORKGROUP, find_bg, pos_bg, from_min, retries, crit)
    assert info["exec_mode"] == "workgroup" and info["q_per_lane"] == 8 and info["waves_per_chain"] == 3, info
    wv, winfo = _run(1025, engine.EXEC_WAVE, find_bg, pos_bg, from_min, retries, crit)
    assert winfo["exec_mode"] == "wave", winfo
    for name in ("num_iter", "num_moves", "attempts", "draws", "converged", "contribs"):
        np.testing.assert_array_equal(getattr(wg, name), getattr(wv, name), err_msg=name)
    for name in ("chisq", "scaling", "fit"):
        np.testing.assert_allclose(getattr(wg, name), getattr(wv, name), rtol=1e-10, err_msg=name)
    _check_against_oracle(wg, refs, crit)
    _check_against_oracle(wv, refs, crit)


@pytest.mark.gpu
@pytest.mark.parametrize("find_bg,pos_bg", CASES_4097)
def test_q_split_kernel_with_sixteen_slots_and_fit_flags_matches_oracle(find_bg, pos_bg):
    refs = _oracle(4097, find_bg, pos_bg, False, 2, 1e-9)
    wg, info = _run(4097, engine.EXEC_WORKGROUP, find_bg, pos_bg, False, 2, 1e-9)
    assert info["exec_mode"] == "workgroup" and info["q_per_lane"] == 16 and info["waves_per_chain"] == 5, info
    _check_against_oracle(wg, refs, 1e-9)
