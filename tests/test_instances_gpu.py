"""Every instance of the wavefront-per-chain and the q-split chain kernels run on the device against exact chains.

One wavefront per chain (csrc/chain_wave.h; kern_lookup.h: MCSAS_WAVE_LOOKUP): 8 built-in models x 12 (q slots per lane, row cache)
pairs x chain_wave_kernel / chain_wave_trace_kernel / chain_wave_batch_kernel<.., GIVEN = false | true> = 576 instances, six per test.
The q-split workgroup (csrc/chain_wide.h; MCSAS_WIDE_LOOKUP): 8 models x 8 / 16 / 32 slots x cold, started, traced cold, traced started
= 96 instances, four per test, at two shapes each.  The matrix, its shapes and its oracle chains are tests/instance_cases.py's;
tests/test_instances_host.py holds every chain to a decisive margin at every step, tests/test_plan_decisions_host.py every shape to
the mode, slot count and wave count its name says.  Here Plan.info confirms what the library picked, and at the module's end the
instances the tests ran are counted (the_tests_ran_every_instance).

No comparison is new.  chain_cases._check_against_oracle and _check_trace against the oracle's chains (counts, steps and draws exact;
sets and recorded values rtol 1e-12; chi² rtol 1e-7; fit rtol 1e-6); chain_cases._same: traced against untraced and a batch against the
single launch bit for bit; a cleared trace leaves none; the records rebuild the final set from the start, exactly for a started chain
(tests/test_trace_gpu.py).  Kholodenko's recorded chains carry no fit: its fit is held by chi² = sum(((I - fit) / sigma)²) / nq
against the device's own chi² (rtol 1e-9, test_random_configurations_all_modes_identical's `direct`), which _check_against_oracle
holds to the oracle's."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import engine
from oracle import mcsas_oracle as O
from chain_cases import FIELDS, WG, _check_against_oracle, _check_trace, _same
import instance_cases as IC

K = IC.CAPACITY
WAVE_FORMS = ("cold", "cold traced", "started traced", "started", "batch cold", "batch started")
WIDE_FORMS = WAVE_FORMS[:4]
RAN = set()          # (family, model, slots, cached rows, form) of every form that passed its checks, as Plan.info named the instance
DONE = set()         # the tests that ran to their end


def _oracle_chains(tag, chains, res, nq):
    """The chains as _check_against_oracle takes them; Kholodenko's get the device's fit once it is held to the device's chi²."""
    if tag != "kholodenko":
        return chains
    q, I, sig = IC.data(nq)
    direct = (((I[:, None] - res.fit) / sig[:, None])**2).sum(axis=0) / nq
    print("chi2 of the reported fit against the reported chi2:", np.abs(direct / res.chisq - 1.).max())
    np.testing.assert_allclose(res.chisq, direct, rtol=1e-9)
    return [dict(c, ref=types.SimpleNamespace(**{**vars(c["ref"]), "fit": res.fit[:, r]})) for r, c in enumerate(chains)]


def _records_rebuild(first, res, exact):
    """The records written in order over the chain's first set, at row step % N, are its final set."""
    N = res.contribs.shape[0]
    for r in range(IC.R):
        rset = np.array(first[r])
        assert 0 < res.trace.count[r] < K
        for i in range(int(res.trace.count[r])):
            rset[res.trace.step[i, r] % N] = res.trace.values[i, :, r]
        if exact:
            assert np.array_equal(rset, res.contribs[:, :, r]), r
        else:
            np.testing.assert_allclose(rset, res.contribs[:, :, r], rtol=1e-12)


def _run(pl):
    pl.launch()
    return pl.fetch()


def _four_forms(tag, nq, cold, hot, family, key):
    """The cold and the started plan through their untraced and traced kernels -> (cold result, started result), both untraced."""
    both = IC.chains(tag, nq)
    _, spec = IC.models(tag)
    P, (N, _) = spec.n_active, IC.budget(tag, nq)
    start = IC.start_array(both)
    plain = _run(cold)
    assert plain.trace is None
    _check_against_oracle(_oracle_chains(tag, both["cold"], plain, nq), plain, P)
    RAN.add((family,) + key + ("cold",))
    cold.set_trace(K)
    traced = _run(cold)
    _same(traced, plain, "cold: traced against untraced")
    _check_trace(both["cold"], traced.trace, K)
    s_cold = IC.seeds(tag, nq)[0]
    _records_rebuild([O.generate_parameters(spec, O.PhiloxStream(s_cold, IC.REP_OFFSET + r, pos=0), N) for r in range(IC.R)], traced, False)
    RAN.add((family,) + key + ("cold traced",))
    cold.set_trace(0)
    hot.set_start(start, rep_first=1)
    hot.set_trace(K)
    started = _run(hot)
    _check_against_oracle(_oracle_chains(tag, both["cont"], started, nq), started, P)
    _check_trace(both["cont"], started.trace, K)
    _records_rebuild([start[:, :, 1 + r] for r in range(IC.R)], started, True)
    assert (started.draws == P * started.num_iter).all()                       # no draws for the given set
    RAN.add((family,) + key + ("started traced",))
    hot.set_trace(0)
    untraced = _run(hot)
    assert untraced.trace is None                                              # a cleared trace writes none
    _same(untraced, started, "started: untraced against traced")
    RAN.add((family,) + key + ("started",))
    return plain, untraced


@pytest.mark.parametrize("tag,qpl,cache", IC.WAVE)
def test_wave_instance(tag, qpl, cache):
    """nq = 64 (QPL - 1) + 37: the instance's last q slot holds 37 points and padding.  Two repetitions at a non-zero rep_offset,
    free-running Philox, to the budget.  The batch holds two cold and two started plans, so each group's table has two entries; the
    second plan of each kind is repetition 1 alone, and equals column 1 of the first plan bit for bit."""
    nq = IC.wave_nq(qpl)
    q, I, sig = IC.data(nq)
    m, _ = IC.models(tag)
    both = IC.chains(tag, nq)
    start = IC.start_array(both)
    plans = [engine.Plan(m.setup(), q, I, sig, IC.engine_settings(tag, nq, engine.EXEC_WAVE, cache, continued=c, n_reps=n, first=f))
             for c, n, f in ((False, IC.R, 0), (True, IC.R, 0), (False, 1, 1), (True, 1, 1))]
    cold, hot, cold1, hot1 = plans
    try:
        for pl in plans:
            info = pl.info
            assert (info["exec_mode"], info["q_per_lane"], info["cached_rows"], info["waves_per_chain"]) == ("wave", qpl, bool(cache), 1), info
        key = (tag, info["q_per_lane"], info["cached_rows"])
        plain, started = _four_forms(tag, nq, cold, hot, "wave", key)
        hot1.set_start(start, rep_first=2)
        engine.launch_batch([cold, hot, cold1, hot1])
        _same(cold.fetch(), plain, "batch against the single launch, cold")
        _same(hot.fetch(), started, "batch against the single launch, started")
        for one, two, form in ((cold1.fetch(), plain, "batch cold"), (hot1.fetch(), started, "batch started")):
            assert one.trace is None
            for name in FIELDS:
                assert np.array_equal(getattr(one, name)[..., 0], getattr(two, name)[..., 1]), (form, name)
            RAN.add(("wave",) + key + (form,))
    finally:
        for pl in plans:
            pl.close()
    DONE.add(("wave", tag, qpl, cache))


@pytest.mark.parametrize("tag,qpl,shape", IC.WIDE)
def test_q_split_instance(tag, qpl, shape):
    """A: the full waves use every slot, the tail wave holds one point (3, 5, 5 waves); B: 8 waves, the last slot of the last wave
    partly filled."""
    nq, waves = IC.WIDE_SHAPES[qpl][shape]
    q, I, sig = IC.data(nq)
    m, _ = IC.models(tag)
    plans = [engine.Plan(m.setup(), q, I, sig, IC.engine_settings(tag, nq, WG, continued=c)) for c in (False, True)]
    try:
        for pl in plans:
            info = pl.info
            assert (info["exec_mode"], info["q_per_lane"], info["waves_per_chain"]) == ("workgroup", qpl, waves), info
        _four_forms(tag, nq, plans[0], plans[1], "q-split", (tag, info["q_per_lane"], None))
    finally:
        for pl in plans:
            pl.close()
    DONE.add(("q-split", tag, qpl, shape))


@pytest.fixture(scope="module", autouse=True)
def the_tests_ran_every_instance():
    """At the module's end: every non-null entry of both lookup tables was run, 96 x 6 wave instances and 24 x 4 q-split instances.
    (Of a selection of the tests: the instances of those that ran to their end.)  A failure here is reported with the last test."""
    yield
    assert len(IC.WAVE) * len(WAVE_FORMS) == 576 and len({(t, q) for t, q, _ in IC.WIDE}) * len(WIDE_FORMS) == 96
    want = {("wave", tag, qpl, bool(cache), form) for fam, tag, qpl, cache in DONE if fam == "wave" for form in WAVE_FORMS}
    want |= {("q-split", tag, qpl, None, form) for fam, tag, qpl, _ in DONE if fam == "q-split" for form in WIDE_FORMS}
    assert want <= RAN, sorted(want - RAN)
    print("tests run to their end: %d of %d; instances: %d wave, %d q-split"
          % (len(DONE), len(IC.WAVE) + len(IC.WIDE), sum(k[0] == "wave" for k in want), sum(k[0] == "q-split" for k in want)))
    if len(DONE) == len(IC.WAVE) + len(IC.WIDE):
        assert sum(k[0] == "wave" for k in want) == 576 and sum(k[0] == "q-split" for k in want) == 96
