"""Series of data sets through one algorithm object: the computational core of the reference's
Calculator (gui/calc.py:271-379) without its log files, HDF5 archive and plots: for every data set
`algo.data = dataset; algo.calc()`, then the moments of every histogram are collected per
(sample, parameter, range, weighting) the way `_updateSeries` does (:331-349)."""
from __future__ import annotations

from collections import OrderedDict


# what run_series(batch_histograms=None) does where a batched pass is possible (the measurement behind it)
BATCH_HISTOGRAMS_DEFAULT = True


def _histograms_batchable(algo, engine):
    """A batched histogram pass needs what McSAS.histogram()'s one-call device path needs: a device model, and no more than
    engine.HISTOGRAM_MAX_CONTRIBS contributions.  The batch call has no partial intensities: when any histogram asks for them
    (Histogram(partialIntensity=...)) the answer is False and the series takes each data set's own McSAS.histogram() call."""
    from .scatteringmodels import setup_from_model
    if algo._partial_todo():
        return False
    return (algo.data is not None and setup_from_model(algo.model, algo.data).model_id != engine.MODEL_HOST
            and algo.numContribs() <= engine.HISTOGRAM_MAX_CONTRIBS)


def run_series(algo, datasets, keys=None, replays=None, overlap=False, batch=False, start=None, batch_histograms=None):
    """-> (results, series).  `results[i]` is `algo.result[0]` of data set i (None when nothing
    converged); `series[(param, lower, upper, yweight)]` is the list of `(key_i, moments.fields)`.
    Every Histogram2D of `algo.histograms2d` adds `series[(paramX, paramY, lowerX, upperX, lowerY, upperY, yweight)]` likewise.
    `keys`: the series key value of each data set (default: its index).  `replays`: per data set, the uniform
    streams of its repetitions (tests replaying the reference: tests/golden/g15_series.npz).  `overlap`: the data sets' analyses
    run side by side on the device instead of one after the other (same results; algo.seed should be set: an unseeded algo draws a
    new seed per data set either way).  `batch`: the Monte-Carlo part of all data sets runs as ONE batch of wavefront-per-chain
    chains (engine.analyse_batch; results as each data set's analysis in that mode alone), the rest as with `overlap`; a model that
    exists only as host code runs one data set after the other instead.
    `start`: the contributions the first attempt of every repetition starts from (McSAS.analyse: an [N][P][R] array; wavefront
    mode, or the q-split workgroup kernel beyond 1024 points: McSAS._check_start_mode) — one array for every data set, a list with one entry per data set (None: cold), or "previous": each data set starts from
    the previous stored result's contributions; the first one, and any after a data set that stored nothing, starts cold.
    "previous" is sequential by nature: with `batch` or `overlap` it raises ValueError.
    `batch_histograms`: with `batch` or `overlap` the chains are done before the first result is stored; True then stores every data
    set's result first and takes all their histograms in ONE library call (engine.histogram_device_batch — the arrays of each data
    set's own McSAS.histogram() call, bit for bit), e.g. `run_series(algo, datasets, batch=True, batch_histograms=True)`; False calls
    McSAS.histogram() per data set.  None: BATCH_HISTOGRAMS_DEFAULT.  A model that exists only as host code, more than
    engine.HISTOGRAM_MAX_CONTRIBS contributions, and the sequential path (neither `batch` nor `overlap`) keep the call per data set."""
    if algo.model is None:
        raise ValueError("no model set")
    previous = isinstance(start, str)
    if previous:
        if start != "previous":
            raise ValueError('run_series: start=%r (an array, a list of arrays / None, or "previous")' % (start,))
        if batch or overlap:
            raise ValueError('run_series: start="previous" chains each data set to the one before; batch / overlap run them together')
    datasets = list(datasets)
    if start is None or previous:
        starts = [None] * len(datasets)
    elif isinstance(start, (list, tuple)):
        if len(start) != len(datasets):
            raise ValueError("run_series: %d start entries for %d data sets" % (len(start), len(datasets)))
        starts = list(start)
    else:
        starts = [start] * len(datasets)
    for data, s in zip(datasets, starts):                    # (what no kernel starts is refused before anything runs)
        algo._check_start_mode(s, data)
    results, series = [], OrderedDict()
    chains = None
    from . import engine
    if batch and algo.model.paramCount():
        algo.stop = False                                    # (as below: once for the batch)
        problems = []
        for i, data in enumerate(datasets):
            algo.data = data
            problems.append(algo._problem(replay=None if replays is None else replays[i], start=starts[i]))
        if all(pr["model"].model_id != engine.MODEL_HOST for pr in problems):
            chains = engine.analyse_batch(problems)
    elif overlap and algo.model.paramCount():
        algo.stop = False                                    # calc() resets it per data set (mcsas.py:152); here once, for the batch
        # the Monte-Carlo part of every data set first, side by side on the device (engine.analyse_many: the data sets' analyses are
        # independent); the loop below then only stores each result and takes its histograms — the same numbers as one after the other
        problems = []
        for i, data in enumerate(datasets):
            algo.data = data
            problems.append(algo._problem(replay=None if replays is None else replays[i], start=starts[i]))
        chains = engine.analyse_many(problems)
    if batch_histograms is None:
        batch_histograms = BATCH_HISTOGRAMS_DEFAULT
    stored = None
    if chains is not None and batch_histograms and _histograms_batchable(algo, engine):
        # the chains are done: store every data set's result, take all their histograms in ONE library call
        # (engine.histogram_device_batch: each set's arrays are those of its own McSAS.histogram() call), then go on as below
        stored, items = [], []
        for i, data in enumerate(datasets):
            algo.data = data
            algo.result = []
            algo._store(chains[i])
            stored.append(algo.result)
            if len(algo.result):
                if all(algo.result[0]['contribs'].shape):    # (histogram() leaves an empty result alone)
                    items.append((i, algo._histogram_item()))
                if algo.stop:                                # (the loop below ends here)
                    break
        device = dict(zip([i for i, _ in items], engine.histogram_device_batch([it for _, it in items])))
    for i, data in enumerate(datasets):
        key = i if keys is None else keys[i]
        algo.data = data
        if stored is not None:
            algo.result, algo.details = stored[i], chains[i]
            if i in device:
                algo._histogram_from_device(device[i])
        elif chains is None:
            prev = results[-1]["contribs"] if previous and results and results[-1] is not None else None
            algo.calc(replay=None if replays is None else replays[i], start=prev if previous else starts[i])
        else:
            # (McSAS.stop is left as the analyses saw it: _store tells "stop pressed" from "criterion not reached" by it)
            algo.result = []
            algo._store(chains[i])
            if len(algo.result):
                algo.histogram()
        if not (isinstance(algo.result, list) and len(algo.result)):
            results.append(None)
            continue
        results.append(algo.result[0])
        for p in algo.model.activeParams():
            for h in p.histograms():
                uid = (p.name(),) + tuple(h.xrange) + (h.yweight,)
                series.setdefault(uid, []).append((key, h.moments.fields))
        for h in getattr(algo, "histograms2d", ()):              # (joint histograms: keys that exist only where one is configured)
            uid = (h.paramX.name(), h.paramY.name()) + tuple(h.xrange) + tuple(h.yrange) + (h.yweight,)
            series.setdefault(uid, []).append((key, h.moments.fields))
        if algo.stop:
            break
    return results, series
