"""McSAS: drop-in mirror of the reference's algorithm object for the Monte-Carlo path.

Same attributes and calls as `mcsas.mcsas.McSAS` (mcsas/mcsas.py:31-179): `McSAS.factory()()`,
`.data`, `.model`, `.result`, `.stop`, the settings as callable parameters (`numContribs()`,
`maxIterations.value()`, `convergenceCriterion.setValue(...)` ...), `calc()`, `analyse()`,
`histogram()`.  `analyse()` runs every repetition as one MI355X kernel launch; nothing is
evaluated on the CPU.  Plotting, HDF5/pickle output and the GUI hooks stay with the reference.
"""
from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np

from . import engine
from .dataobj import DataSets
from .parameter import isActiveFitParam, partial_intensities
from .scatteringmodels import (setup_from_model, host_model_calc, is_batch_model, batch_model_calc, batch_clip,
                               refuse_batch_smearing)


# what McSAS.histogram() does for a calcIntensityBatch model where McSAS.deviceRowsHistogram is None: the rows stay on the device
# (engine.histogram_device_rows); False: the rows are downloaded and the limits taken in numpy (the measurement behind it)
DEVICE_ROWS_HISTOGRAM_DEFAULT = True


def _q_on_device(q):
    """`at(pset)`: q as a flat torch tensor on the device of `pset`, made at the first call and kept (torch is imported there, not
    with the package): what a calcIntensityBatch model is handed beside the parameter sets of every round"""
    kept = []

    def at(pset):
        if not kept:
            import torch
            kept.append(torch.as_tensor(np.ascontiguousarray(q, dtype=np.float64), device=pset.device).reshape(-1))
        return kept[0]
    return at


class _Setting(object):
    """Algorithm parameter with the reference's accessors (`p()`, `p.value()`, `p.setValue(v)`)."""

    def __init__(self, name, default, valueRange=None):
        self._name, self._value, self._range = name, default, valueRange

    def name(self):
        return self._name

    def value(self):
        return self._value

    __call__ = value

    def setValue(self, v):
        if self._range is not None and not isinstance(v, bool):
            v = min(max(v, self._range[0]), self._range[1])
        self._value = type(self._value)(v) if not isinstance(self._value, bool) else bool(v)


# mcsas/mcsasparameters.json:2-103
_DEFAULTS = (
    ("numContribs", 300, (1, 1e6)), ("numReps", 10, (1, 1e6)), ("maxIterations", 1e5, (1, 1e100)),
    ("compensationExponent", 0.6666666, None), ("convergenceCriterion", 1.0, (0, np.inf)),
    ("findBackground", True, None), ("positiveBackground", False, None),
    ("startFromMinimum", False, None), ("maxRetries", 5, (1, 100)), ("showIncomplete", False, None),
)


class _HostPartial(object):
    """The partial intensities of the histograms `todo` [(paramIndex, histogram)] in numpy, a repetition at a time
    (parameter.partial_intensities: the operation order of csrc/hist_partial_kernel.h)."""

    def __init__(self, todo, nq, numReps):
        self.todo = list(todo)
        for _, h in self.todo:
            h._setXLowerEdge()
        self.range = [np.zeros((nq, numReps)) for _ in self.todo]
        self.bins = [np.zeros((h.binCount, nq, numReps)) if h.partialIntensity == "bins" else None for _, h in self.todo]

    def add(self, ri, rows, pset, scale):
        for k, (pi, h) in enumerate(self.todo):
            rng, bins = partial_intensities(rows, pset[:, pi], scale, min(h.xrange), max(h.xrange), h.xLowerEdge, self.bins[k] is not None)
            self.range[k][:, ri] = rng
            if bins is not None:
                self.bins[k][:, :, ri] = bins

    def finish(self):
        for k, (pi, h) in enumerate(self.todo):
            h.setIntensity(self.range[k], self.bins[k])


class McSAS(object):
    data = None
    model = None
    result = None

    @classmethod
    def factory(cls):                                        # mcsas.py:143-147
        return cls

    def __init__(self, seed=None, device=-1, wavesPerChain=0, execMode=0):
        """`device`: a HIP device ordinal (-1: the current device) or a list of them — the repetitions are then spread
        over those GPUs by the library (contiguous blocks, mcsas_hip.h: n_devices / devices), results in repetition order
        as if one device had run them; `histogram()` uses the first of the list."""
        for name, default, rng in _DEFAULTS:
            setattr(self, name, _Setting(name, default, rng))
        self.seed = seed
        self.devices = tuple(int(d) for d in device) if isinstance(device, (list, tuple)) else ()
        self.device = self.devices[0] if self.devices else int(device)
        self.wavesPerChain = wavesPerChain
        self.execMode = execMode
        self._stop = C.c_int32(0)
        self.details = None
        self.hostRowWindow = 64          # proposals evaluated ahead per chain for models that exist only as Python (mcsas_hip.h)
        self.deviceRowsHistogram = None  # histogram() of a calcIntensityBatch model on the device: None = DEVICE_ROWS_HISTOGRAM_DEFAULT
        self.histograms2d = []           # parameter.Histogram2D objects over pairs of the model's active parameters: histogram() fills them

    # McSAS.stop is polled once per step in the reference (mcsas.py:357); here the word is
    # forwarded to the running kernel by the library
    @property
    def stop(self):
        return bool(self._stop.value)

    @stop.setter
    def stop(self, flag):
        self._stop.value = 1 if flag else 0

    def _check_start_mode(self, start, data=None):
        """The execution mode a started analysis of `data` (default: the current data) asks for, or None without a start
        (engine.kernel_mode: here a start picks the workgroup mode where execMode leaves the choice open and no other kernel takes
        the data).  ValueError where no kernel takes a start."""
        if start is None:
            return None
        data = self.data if data is None else data
        nq = 0 if data is None else int(np.size(data.q))
        return engine.kernel_mode("start", self.execMode, nq, "McSAS", auto_beyond_wave=True, mode_word="execMode", q_word="points")

    def _check_trace_mode(self, trace, data=None):
        """The execution mode a traced analysis of `data` (default: the current data) asks for, or None without a trace
        (engine.kernel_mode; include/mcsas_hip.h: mcsas_hip_analyse_traced).  The trace never picks the mode: ValueError where no
        traced kernel runs under execMode, for a model that exists only as host code and for a device list."""
        if trace is None:
            return None
        data = self.data if data is None else data
        nq = 0 if data is None else int(np.size(data.q))
        if int(trace) < 1:
            raise ValueError("McSAS: trace is the number of moves kept per repetition (>= 1), got %r" % (trace,))
        mode = engine.kernel_mode("trace", self.execMode, nq, "McSAS", mode_word="execMode", q_word="points")
        if self.devices:
            raise ValueError("McSAS: a trace is kept on one device; the device list %r was given" % (self.devices,))
        if self.model is not None and setup_from_model(self.model, data).model_id == engine.MODEL_HOST:
            raise ValueError("McSAS: a model that exists only as host code keeps no trace (it runs through host-evaluated rows)")
        return mode

    def calc(self, **kwargs):                                # mcsas.py:149-179
        """`trace=K`: keeps the first K accepted moves of every repetition (step, chi-squared, new values: what the reference logs
        as "good iter", mcsas.py:385-390) under `algo.result[0]['trace']`; combines with `start=`.
        `start=`: an [N][P][R] array of contributions, typically an earlier `algo.result[0]['contribs']`: the first attempt of
        every repetition starts from it instead of a random set — to continue a run that ended at maxIterations, to refine a result
        to a tighter criterion, or to warm-start from a neighbouring data set's result (see analyse)."""
        self._check_start_mode(kwargs.get("start"))
        self._check_trace_mode(kwargs.get("trace"))
        self.result = []
        self.stop = False
        assert self.data is not None
        if self.model is None:
            raise ValueError("McSAS.model is not set")
        if not self.model.paramCount():
            logging.warning("No parameters to analyse given! Breaking up.")
            return
        self.analyse(replay=kwargs.get("replay"), start=kwargs.get("start"), trace=kwargs.get("trace"))   # (replay: tests feed the uniform stream the reference consumed)
        if not len(self.result):
            return
        self.histogram()

    def _settings(self, numContribs, numReps):
        seed = self.seed
        if seed is None:                                     # reference: unseeded global MT19937
            seed = int.from_bytes(os.urandom(8), "little")
        return engine.Settings(
            n_contrib=int(numContribs), n_reps=int(numReps), max_iter=self.maxIterations.value(),
            comp_exp=self.compensationExponent(), conv_crit=self.convergenceCriterion(),
            find_background=self.findBackground.value(), positive_background=self.positiveBackground.value(),
            start_from_minimum=self.startFromMinimum(), max_retries=int(self.maxRetries()),
            show_incomplete=self.showIncomplete(), seed=seed, device=self.device, devices=self.devices,
            waves_per_chain=self.wavesPerChain, exec_mode=self.execMode)

    def analyse(self, replay=None, start=None, trace=None):  # mcsas.py:191-285
        """`start`: [numContribs][active parameters][>= numReps] — mcFit's rset of the first attempt of each repetition, in place of
        generateParameters(numContribs) (mcsas.py:317); later attempts draw a fresh set as always.  A start runs one wavefront per chain
        for this call, or the q-split workgroup kernel (_check_start_mode; include/mcsas_hip.h: mcsas_hip_analyse_from); an explicit
        execMode of pipeline, or of workgroup with up to 1024 points, raises ValueError.
        `trace`: K >= 1 stores the first K accepted moves of every repetition's last attempt under result[0]['trace'] (count, chisq0,
        step[K][R], chisq[K][R], values[K][P][R]: engine.ChainTrace); one wavefront per chain, or the q-split workgroup kernel where
        execMode asks for it (_check_trace_mode)."""
        if isinstance(self.data, DataSets):
            return self._analyse_sets(replay, start, trace)
        trace_mode = self._check_trace_mode(trace)
        if self.result is None:
            self.result = []
        data, model = self.data, self.model
        if not any(isActiveFitParam(p) for p in model.params()):
            numContribs, numReps = 1, 1                      # mcsas.py:198-199: nothing active, nothing to fit
        else:
            numContribs, numReps = self.numContribs(), self.numReps()
        pr = self._problem(numContribs, numReps, replay, start)
        if trace is not None:
            pr["st"].exec_mode = trace_mode                  # (with a start: the mode _check_start_mode gave, wherever a trace is taken)
        if pr["model"].model_id == engine.MODEL_HOST:
            # a model with Python formfactor / volume only: its rows are evaluated here, by the model's own calcIntensity with the
            # set-value-and-restore semantics of ScatteringModel.calc (scatteringmodel.py:86-104); the device does the rest
            c = self.compensationExponent()
            if is_batch_model(model):
                # ... or with calcIntensityBatch in torch: the rows of a whole round in one call on the device, where the library
                # generated the proposals and decides on them (mcsas_hip_analyse_device_rows); the clipping of setValue on a copy
                refuse_batch_smearing(model, data)
                qdev = _q_on_device(pr["q"])

                def rows_on_device(pset, out):
                    return model.calcIntensityBatch(qdev(pset), batch_clip(model, pset), c)[0]
                res = engine.analyse_device_rows(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"], rows_on_device,
                                                 replay=pr["replay"], stop=pr["stop"], window=self.hostRowWindow)
            else:
                def rows(pset):
                    return host_model_calc(model, data, pset, c, want_rows=True)[4]
                res = engine.analyse_host_rows(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"], rows,
                                               replay=pr["replay"], stop=pr["stop"], window=self.hostRowWindow)
        else:
            res = engine.analyse(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"],
                                 replay=pr["replay"], stop=pr["stop"], smear=pr["smear"], start=pr.get("start"), trace=trace)
        self._store(res, numReps)
        if trace is not None and res.trace is not None and len(self.result):
            self.result[0]['trace'] = res.trace.asdict()

    def _analyse_sets(self, replay=None, start=None, trace=None):
        """analyse() where `data` is a DataSets: one population fitted to all members at once, each with a scale and a background of
        its own (engine.analyse_sets).  result[0] keeps its keys, the q-indexed ones over the members one after the other (scaling and
        background: member 0's), and gains 'sets': per member a dict of `slice` (where it lies among the points), `scaling` and
        `background` (mean, std over the repetitions) and `chisq` (per repetition: the sum over the member / its number of points),
        and 'setsScale': "per_set", or "shared" where DataSets.sharedScale asks for one scale for all members.
        A start and a trace are refused, and so is everything engine.analyse_sets refuses."""
        if start is not None or trace is not None:
            raise ValueError("McSAS: the joint fit of a DataSets takes no %s" % ("start" if start is not None else "trace"))
        if self.result is None:
            self.result = []
        data, model = self.data, self.model
        if not any(isActiveFitParam(p) for p in model.params()):
            raise ValueError("McSAS: the joint fit of a DataSets needs an active fit parameter")
        numReps = self.numReps()
        st = self._settings(self.numContribs(), numReps)
        scale = "shared" if getattr(data, "sharedScale", False) else "per_set"
        mode = dict(scale=scale) if scale != "per_set" else {}   # (the per-set call is what it was, argument for argument)
        res = engine.analyse_sets(setup_from_model(model, data), data.triples(), st, replay=replay, stop=self._stop, **mode)
        self._store(res, numReps)
        if len(self.result):
            ddof = 1 if numReps > 1 else 0
            self.result[0]['setsScale'] = scale
            self.result[0]['sets'] = [dict(slice=sl, scaling=(res.set_scaling[s].mean(), res.set_scaling[s].std(ddof=ddof)),
                                           background=(res.set_background[s].mean(), res.set_background[s].std(ddof=ddof)),
                                           chisq=res.set_chisq[s].copy()) for s, sl in enumerate(res.slices)]

    def _problem(self, numContribs=None, numReps=None, replay=None, start=None):
        """What analyse() hands to the library for the current data / model / settings (engine.analyse_many takes a list of these).
        With a `start` (see analyse) the problem asks for the mode of _check_start_mode and carries the checked array under "start"."""
        data, model = self.data, self.model
        if isinstance(data, DataSets):
            raise ValueError("McSAS: the joint fit of a DataSets runs through analyse() / calc() alone; it has no plan, batch or series form")
        if numContribs is None:
            active = any(isActiveFitParam(p) for p in model.params())
            numContribs, numReps = (self.numContribs(), self.numReps()) if active else (1, 1)
        smear = data.smearArgs(model) if hasattr(data, "smearArgs") else None   # sasmodel.py:56-60
        pr = dict(model=setup_from_model(model, data), q=data.q, intensity=data.f.binnedData, sigma=data.f.binnedDataU,
                  st=self._settings(numContribs, numReps), replay=replay, stop=self._stop, smear=smear)
        if start is not None and pr["model"].n_active > 0:
            mode = self._check_start_mode(start)
            a = engine._check_start(start, pr["model"], pr["st"], "McSAS.analyse")
            engine._start_columns(a, pr["st"], 0, "McSAS.analyse")
            pr["st"].exec_mode = mode
            pr["start"] = a
        return pr

    def _store(self, res, numReps=None):
        """The second half of analyse() (mcsas.py:221-285): warnings, active values, the result dictionary."""
        data, model = self.data, self.model
        if self.result is None:
            self.result = []
        if numReps is None:
            numReps = res.contribs.shape[2]
        self.details = res
        if (res.converged == 0).any():                       # mcsas.py:221-230 / :240-245
            if self.stop:
                logging.warning("Stop button pressed, exiting...")
            else:
                logging.warning("Could not reach optimization criterion within {0} attempts, exiting..."
                                .format(self.maxRetries() + 2))
            if not self.showIncomplete():
                return
        contribs = res.contribs
        for nr in range(numReps):                            # mcsas.py:434-437
            for idx, param in enumerate(model.activeParams()):
                param.setActiveVal(contribs[:, idx, nr].copy(), index=nr)
        meas = res.fit.reshape(1, data.count, numReps)       # contribMeasVal, mcsas.py:210
        ddof = 1 if numReps > 1 else 0
        self.result.append(dict(
            contribs=contribs,
            fitMeasValMean=meas.mean(axis=2), fitMeasValStd=meas.std(axis=2),
            fitX0=data.x0.binnedData, dataX0=data.x0.binnedData,
            dataMean=data.f.binnedData, dataStd=data.f.binnedDataU,
            scaling=(res.scaling.mean(), res.scaling.std(ddof=ddof)),
            background=(res.background.mean(), res.background.std(ddof=ddof)),
            times=res.seconds, numIter=res.num_iter.astype(float).mean()))

    def histogram(self, contribs=None):                      # mcsas.py:445-615
        """With a DataSets as `data`: histogramSet an index and sharedScale False — everything below runs against ONE member through
        the single-set path: its scale fit is the joint fit's for that member, and the visibility limits are those as seen by that
        set.  histogramSet "all" or sharedScale True — _histogram_sets: the points of all members in one device call."""
        if isinstance(self.data, DataSets):
            sets = self.data
            if sets.jointHistogram():
                return self._histogram_sets(contribs)
            self.data = sets.histogramMember()
            try:
                return self.histogram(contribs)
            finally:
                self.data = sets
        if not isinstance(self.result, list) or not len(self.result):
            logging.info("There are no results to histogram, breaking up.")
            return
        if contribs is None:
            contribs = self.result[0]['contribs']
        if not all(np.array(contribs.shape, dtype=bool)):
            return
        numContribs, dummy, numReps = contribs.shape
        data, model = self.data, self.model
        setup = setup_from_model(model, data)
        smear = data.smearArgs(model) if hasattr(data, "smearArgs") else None
        c = self.compensationExponent()
        sig = np.array(data.f.binnedDataU, dtype=float)
        if setup.model_id == engine.MODEL_HOST:
            on_device = DEVICE_ROWS_HISTOGRAM_DEFAULT if self.deviceRowsHistogram is None else self.deviceRowsHistogram
            if is_batch_model(model) and numContribs <= engine.HISTOGRAM_MAX_CONTRIBS and on_device:
                # calcIntensityBatch in torch: the rows of a round of repetitions in one call on the device, where the library laid
                # the sets out and takes the fit, the limits, the fractions and the histograms from them (mcsas_hip_histogram_device_rows)
                refuse_batch_smearing(model, data)
                qdev = _q_on_device(data.q)

                def rows_on_device(pset):
                    return model.calcIntensityBatch(qdev(pset), batch_clip(model, pset), c)
                item = self._histogram_item(setup, None, contribs)
                del item["comp_exp"], item["smear"]
                self._histogram_from_device(engine.histogram_device_rows(row_fn=rows_on_device, **item), contribs)
                self._partial_on_host(contribs, setup, smear, [(pi, h) for pi, h in self._partial_todo() if not h.partialOnDevice()])
                return
            # rows by the model's own calcIntensity (:552, :577-578), the fit on the device (:559), the visibility limits in numpy (:575-590)
            scalingFactors = np.zeros((2, numReps))
            vsets = np.zeros((numContribs, numReps)); wsets = np.zeros((numContribs, numReps)); ssets = np.zeros((numContribs, numReps))
            mv = np.zeros((numContribs, numReps))
            # (a batch model: the sets of a block of repetitions in one calcIntensityBatch call, at most ~256 MB of rows at a time)
            batch = is_batch_model(model)
            per_block = max(1, (256 << 20) // (8 * data.count * numContribs)) if batch else 1
            partial = _HostPartial(self._partial_todo(), data.count, numReps)      # (from the rows held here anyway)
            for ri in range(numReps):
                if batch:
                    if ri % per_block == 0:
                        r1 = min(numReps, ri + per_block)
                        sets = np.ascontiguousarray(np.moveaxis(contribs[:, :, ri:r1], 2, 0)).reshape((r1 - ri) * numContribs, -1)
                        block = [a.reshape(r1 - ri, numContribs, -1) for a in batch_model_calc(model, data, sets, c, want_rows=True,
                                                                                             device=self.device)[1:]]
                    k = ri % per_block
                    vsets[:, ri], wsets[:, ri], ssets[:, ri], rows = block[0][k, :, 0], block[1][k, :, 0], block[2][k, :, 0], block[3][k]
                    cum = np.cumsum(rows, axis=0)[-1]        # (rows added in order, scatteringmodel.py:90-101)
                else:
                    cum, vsets[:, ri], wsets[:, ri], ssets[:, ri], rows = host_model_calc(model, data, contribs[:, :, ri], c, want_rows=True)
                sc, _, _ = engine.bgfit(data.f.binnedData, sig, cum, self.findBackground.value(), self.positiveBackground.value(),
                                        num_params=model.activeParamCount(), device=self.device)
                scalingFactors[:, ri] = sc
                vf_r = wsets[:, ri] * sc[0] / vsets[:, ri]
                for ci in range(numContribs):
                    part = sc[0] * rows[ci]
                    nz = part != 0.
                    mv[ci, ri] = (sig[nz] * vf_r[ci] / part[nz]).min()
                partial.add(ri, rows, contribs[:, :, ri], sc[0])
            self._histogram_tail(contribs, scalingFactors, vsets, wsets, ssets, mv)
            partial.finish()
            return
        # Everything on the device in one call (mcsas_hip_histogram): model.calc, the scale / background fit, the visibility
        # limits, the fractions, and per configured histogram the bins, CDF and moments of every repetition — their mean / std over
        # the repetitions is taken here.  (More than engine.HISTOGRAM_MAX_CONTRIBS contributions: the two-step path below.)
        if numContribs <= engine.HISTOGRAM_MAX_CONTRIBS:
            item = self._histogram_item(setup, smear, contribs)
            self._histogram_from_device(engine.histogram_device(**item), contribs)
            self._partial_on_host(contribs, setup, smear, [(pi, h) for pi, h in self._partial_todo() if not h.partialOnDevice()])
            return
        # model.calc, the scale/background fit and the N single-row visibility limits of every repetition
        # (:552, :559, :575-590): one library call for all of them
        scalingFactors, vsets, wsets, ssets, mv = engine.histogram_prep(
            setup, data.q, data.f.binnedData, sig, contribs, c, self.findBackground.value(),
            self.positiveBackground.value(), device=self.device, smear=smear)
        self._histogram_tail(contribs, scalingFactors, vsets, wsets, ssets, mv)
        self._partial_on_host(contribs, setup, smear, self._partial_todo())

    def _histogram_sets(self, contribs=None):
        """histogram() over the points of all members of a DataSets (engine.histogram_sets): per repetition every member is fitted to
        the summed intensity — a scale per member, or one for all with DataSets.sharedScale —, volume fractions are by member
        scaleSet's scale (the shared one), and a contribution's visibility limit is the lowest any member named by histogramSet
        gives it.  result[0]['scalingFactors'] is the reference pair.  Partial intensities and more than
        engine.HISTOGRAM_MAX_CONTRIBS contributions are refused: there is no single-member path to fall back to."""
        if not isinstance(self.result, list) or not len(self.result):
            logging.info("There are no results to histogram, breaking up.")
            return
        if contribs is None:
            contribs = self.result[0]['contribs']
        if not all(np.array(contribs.shape, dtype=bool)):
            return
        sets, model = self.data, self.model
        if self._partial_todo():
            raise ValueError("McSAS.histogram: Histogram(partialIntensity=...) is not offered where a DataSets is histogrammed over all "
                             "members (histogramSet=\"all\" or sharedScale=True); use histogramSet=<index> with sharedScale=False")
        if contribs.shape[0] > engine.HISTOGRAM_MAX_CONTRIBS:
            raise ValueError("McSAS.histogram: %d contributions; the histogram of a DataSets over all members takes at most %d"
                             % (contribs.shape[0], engine.HISTOGRAM_MAX_CONTRIBS))
        out = engine.histogram_sets(setup_from_model(model, sets), sets.triples(), contribs, self.compensationExponent(),
                                    [h.deviceSpec(pi) for pi, h in self._histogram_todo()], find_background=self.findBackground.value(),
                                    device=self.device, scale="shared" if sets.sharedScale else "per_set", ref_set=sets.scaleSet,
                                    visible=sets.visibleSets())
        self._histogram_from_device(out[:3], contribs)

    def _histogram_todo(self):
        return [(pi, h) for pi, param in enumerate(self.model.activeParams()) for h in param.histograms()]

    def _partial_todo(self):
        """the histograms that ask for partial intensities (Histogram(partialIntensity=...))"""
        return [(pi, h) for pi, h in self._histogram_todo() if getattr(h, "partialIntensity", None)]

    def _partial_on_host(self, contribs, setup, smear, todo):
        """The partial intensities the device call did not take — more than engine.HISTOGRAM_MAX_CONTRIBS contributions, more than
        engine.HISTOGRAM_PARTIAL_MAX_BINS bins, edges that are not finite — in numpy (parameter.partial_intensities) from the rows of
        a repetition at a time: engine.model_calc(want_rows=True), or the host model's own.  After the histograms have their moments
        and result[0]['scalingFactors'] is set; with nobody asking nothing runs."""
        if not todo:
            return
        data, model, c = self.data, self.model, self.compensationExponent()
        numReps = contribs.shape[2]
        scale = self.result[0]['scalingFactors'][0]
        partial = _HostPartial(todo, data.count, numReps)
        for ri in range(numReps):
            pset = np.ascontiguousarray(contribs[:, :, ri])
            if setup.model_id != engine.MODEL_HOST:
                rows = engine.model_calc(setup, data.q, pset, c, want_rows=True, device=self.device, smear=smear)[4]
            elif is_batch_model(model):
                rows = batch_model_calc(model, data, pset, c, want_rows=True, device=self.device)[4]
            else:
                rows = host_model_calc(model, data, pset, c, want_rows=True)[4]
            partial.add(ri, np.asarray(rows).reshape(len(pset), -1), pset, scale[ri])
        partial.finish()

    def _histogram_item(self, setup=None, smear=None, contribs=None):
        """engine.histogram_device's arguments (by name) for the stored result with the current data, model and histograms
        (run_series hands a list of these to engine.histogram_device_batch)."""
        data, model = self.data, self.model
        if setup is None:
            setup = setup_from_model(model, data)
            smear = data.smearArgs(model) if hasattr(data, "smearArgs") else None
        if contribs is None:
            contribs = self.result[0]['contribs']
        return dict(model=setup, q=data.q, intensity=data.f.binnedData, sigma=np.array(data.f.binnedDataU, dtype=float),
                    contribs=contribs, comp_exp=self.compensationExponent(),
                    specs=[h.deviceSpec(pi) for pi, h in self._histogram_todo()], find_background=self.findBackground.value(),
                    positive_background=self.positiveBackground.value(), device=self.device, smear=smear)

    def _histogram_from_device(self, triple, contribs=None):
        """Takes over what engine.histogram_device returned for the stored result (or for `contribs`)."""
        scalingFactors, fractions, res = triple
        self.result[0]['scalingFactors'] = scalingFactors
        self.fractions = fractions
        for (pi, h), r in zip(self._histogram_todo(), res):
            h.setFromDevice(r)
        self._histograms2d_calc(contribs)

    def _histograms2d_calc(self, contribs=None):
        """The joint histograms of `histograms2d` from the contributions and `self.fractions`, where histogram() ends: on the device
        in one call (engine.histogram2d_device) those with no more than engine.HISTOGRAM_MAX_CONTRIBS contributions and
        engine.HISTOGRAM2D_MAX_CELLS cells, in numpy (Histogram2D.calc) the others.  With an empty list nothing runs."""
        if not self.histograms2d:
            return
        if contribs is None:
            contribs = self.result[0]['contribs']
        active = list(self.model.activeParams())
        on_device, on_host = [], []
        for h in self.histograms2d:
            idx = []
            for p in (h.paramX, h.paramY):
                where = [i for i, a in enumerate(active) if a is p] or [i for i, a in enumerate(active) if a.name() == p.name()]
                if not where:
                    raise ValueError("McSAS.histograms2d: parameter %r is not among the model's active parameters (%s)"
                                     % (p.name(), ", ".join(a.name() for a in active)))
                idx.append(where[0])
            fits = contribs.shape[0] <= engine.HISTOGRAM_MAX_CONTRIBS and h.binCount[0] * h.binCount[1] <= engine.HISTOGRAM2D_MAX_CELLS
            (on_device if fits else on_host).append((h, idx[0], idx[1]))
        if on_device:
            res = engine.histogram2d_device(contribs, self.fractions, [h.deviceSpec(ix, iy) for h, ix, iy in on_device], device=self.device)
            for (h, ix, iy), r in zip(on_device, res):
                h.setFromDevice(r)
        for h, ix, iy in on_host:
            h.calc(contribs, ix, iy, self.fractions)

    def _histogram_tail(self, contribs, scalingFactors, vsets, wsets, ssets, mv):
        """mcsas.py:561-615 from the per-contribution volumes / weights / surfaces and visibility limits of every repetition."""
        model = self.model
        vf = wsets * scalingFactors[0][None, :] / vsets          # modeldata.py:57-61
        nf = vf / vsets
        qf = vf * vsets
        sf = nf * ssets
        mn = mv / vsets                                      # :591-594
        mq = mn * mv * mv
        ms = mn * ssets
        # normalisation per repetition (:596-604); cumsum adds in the order of the reference's builtin sum()
        for frac, lim in ((nf, mn), (qf, mq), (sf, ms)):
            tot = np.cumsum(frac, axis=0)[-1]
            nz = tot != 0
            frac[:, nz] /= tot[nz]; lim[:, nz] /= tot[nz]
        fractions = dict(vol=(vf, mv), num=(nf, mn), int=(qf, mq), surf=(sf, ms))
        self.result[0]['scalingFactors'] = scalingFactors
        self.fractions = fractions
        for paramIndex, param in enumerate(model.activeParams()):
            param.histograms().calc(contribs, paramIndex, fractions)
        self._histograms2d_calc(contribs)
