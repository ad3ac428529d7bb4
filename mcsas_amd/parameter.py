"""Parameter / FitParameter / NumberGenerator / Histogram: the slice of the reference's parameter
system the hot path and its callers touch, with the reference's method names.

  reference: bases/algorithm/parameter.py:205-330,390-525 (ParameterBase/Numerical/Float),
             utils/parameter.py:577-743 (FitParameter*), bases/algorithm/numbergenerator.py,
             utils/parameter.py:187-538 (Histogram) and :20-184 (Moments, VectorResult).
Values are SI throughout (the reference converts display units on entry; units.py is out of scope).
Histogram binning is host-side post-processing; the per-contribution intensities
it needs come from the GPU (engine.model_calc / engine.observability).
"""
from __future__ import annotations

import numpy as np


# ------------------------------------------------------------------ number generators
class NumberGenerator(object):
    """numbergenerator.py:14-22.  `kind` is the MCSAS_GEN_* code the kernels implement."""
    kind = 0

    @classmethod
    def get(cls, count=1):
        raise NotImplementedError


class RandomUniform(NumberGenerator):
    kind = 0

    @classmethod
    def get(cls, count=1):                                   # numbergenerator.py:28-31
        return np.random.uniform(size=count)


class RandomExponential(NumberGenerator):
    kind = 1
    lower, upper = 0., 1.

    @classmethod
    def get(cls, count=1):                                   # numbergenerator.py:168-175
        rs = 10**(np.random.uniform(cls.lower, cls.upper, count))
        return (rs - 1) / (10**(cls.upper - cls.lower))


class RandomExponential1(RandomExponential):
    pass


class RandomExponential2(RandomExponential):
    kind = 2
    upper = 2.


class RandomExponential3(RandomExponential):
    kind = 3
    upper = 3.


def generator_kind(gen):
    """MCSAS_GEN_* of a generator class: ours by attribute, the reference's by class name."""
    k = getattr(gen, "kind", None)
    if k is not None:
        return int(k)
    name = getattr(gen, "__name__", str(gen))
    table = {"RandomUniform": 0, "RandomExponential": 1, "RandomExponential1": 1,
             "RandomExponential2": 2, "RandomExponential3": 3}
    if name not in table:
        raise ValueError("generator %s has no device implementation" % name)
    return table[name]


# ------------------------------------------------------------------ parameters
class Parameter(object):
    """A named model value with a valueRange; callable like the reference's (`p()` -> value)."""

    def __init__(self, name, value, displayName=None, valueRange=None, **_ignored):
        self._name = name
        self._valueRange = (-np.inf, np.inf)                  # a parameter declared without a range has none
        self._displayName = displayName or name
        self._value = value
        if valueRange is not None:
            self.setValueRange(valueRange)                    # (clips the constructor's value into the range like the reference)

    def name(self):
        return self._name

    def displayName(self):
        return self._displayName

    def value(self):
        return self._value

    __call__ = value

    def valueRange(self):
        return self._valueRange

    def setValueRange(self, newRange):
        # bases/algorithm/parameter.py:420-433: infinities are stored as +-1e200 ("as good as inf")
        self._valueRange = (max(min(newRange), -1e200), min(max(newRange), 1e200))
        # ... and the current value is brought into the new range (:431-433: setValue(clip()))
        v = getattr(self, "_value", None)
        if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)):
            self._value = type(v)(np.clip(v, self._valueRange[0], self._valueRange[1])) if isinstance(v, (int, np.integer)) else float(np.clip(v, self._valueRange[0], self._valueRange[1]))

    def min(self):
        return self._valueRange[0]

    def max(self):
        return self._valueRange[1]

    def clip(self, value=None):                              # parameter.py:489-495
        if value is None:
            value = self._value
        return np.clip(value, self.min(), self.max())

    def setValue(self, newValue, clip=True):                 # parameter.py:405-414
        if newValue is None:
            return
        if isinstance(newValue, (bool, np.bool_)):
            self._value = bool(newValue)
            return
        self._value = float(self.clip(newValue)) if clip else float(newValue)

    def isActive(self):
        return False


class Histograms(list):
    def calc(self, *args):                                   # utils/parameter.py:562-565
        for h in self:
            h.calc(*args)


class FitParameter(Parameter):
    """utils/parameter.py:577-743: adds isActive / activeRange / generator / histograms / activeValues."""

    def __init__(self, name, value, displayName=None, valueRange=None, activeRange=None,
                 generator=RandomUniform, **kw):
        super().__init__(name, value, displayName, valueRange, **kw)
        self._isActive = False
        self._activeRange = None
        self._generator = generator
        self._histograms = Histograms()
        self._histograms2d = []
        self._activeValues = []
        if activeRange is not None:
            self.setActiveRange(activeRange)

    def isActive(self):
        return self._isActive

    def setIsActive(self, isActive):
        self._isActive = bool(isActive)

    setActive = setIsActive

    def setActiveRange(self, newRange):                      # utils/parameter.py:615-624
        if len(newRange) != 2:
            raise ValueError("Active ranges have to consist of two values!")
        r = self.clip(np.asarray(newRange, dtype=float))
        self._activeRange = (float(min(r)), float(max(r)))
        for h in self._histograms:
            h.updateRange()
        for h in self._histograms2d:                          # (Histogram2D: the joint histograms this parameter is an axis of)
            h.updateRange()

    def activeRange(self):
        return self._activeRange if self._activeRange is not None else self.valueRange()

    def generator(self):
        return self._generator

    def setGenerator(self, gen):
        self._generator = gen if isinstance(gen, type) else RandomUniform

    def histograms(self):
        return self._histograms

    def activeValues(self):
        return self._activeValues

    def activeVal(self, index=None):
        if index is None:
            return self._activeValues
        return self._activeValues[index % len(self._activeValues)]

    def setActiveVal(self, val, index=None):                 # utils/parameter.py:666-694
        if not self.isActive():
            return
        vals = self._activeValues
        if index is None:
            index = len(vals)
        elif index < 0:
            index = len(vals) + index + 1
        while len(vals) <= index:
            vals.append(None)
        vals[index] = val

    def generate(self, lower=None, upper=None, count=1):     # utils/parameter.py:715-728, parameter.py:66-84
        lo = min(self.activeRange()) if lower is None else lower
        hi = max(self.activeRange()) if upper is None else upper
        lo, hi = max(self.min(), lo), min(self.max(), hi)
        return self._generator.get(count) * (hi - lo) + lo


def isActiveFitParam(param):
    """utils/parameter.py:573-576; duck-typed so the reference's own parameter objects work too."""
    f = getattr(param, "isActive", None)
    return bool(f()) if callable(f) else False


# ------------------------------------------------------------------ histogram (post-fit)
class VectorResult(object):
    """utils/parameter.py:156-184."""

    def __init__(self, vec):
        assert vec.ndim == 2
        self.full = vec
        self.mean = vec.mean(axis=1)
        self.std = vec.std(axis=1, ddof=1 if len(vec) > 1 else 0)


def partial_intensities(rows, x, A, lower, upper, edges=None, bins=False):
    """The partial intensities of one repetition in numpy: the transcription of hist_partial_kernel's operation order
    (csrc/hist_partial_kernel.h), equal to it bit for bit.  `rows` [N][nq]: the contributions' intensity rows; `x` [N]: their values
    of the histogram's parameter; `A`: the repetition's scale.  Returns (range[nq], bin[n_bin][nq] or None):
        range[k]  = A * sum_c rows[c][k] over lower < x_c < upper (strict: the mask of the moments)
        bin[b][k] = A * sum_c rows[c][k] over edges[b] <= x_c < edges[b+1] and x_c < edges[-1] (Histogram.calc's members)
    Each sum is a cumulative sum down the contributions, in order, from +0.0, and is multiplied by A once, at the end.  The
    contributions outside add +0.0, which leaves a running sum that began at +0.0 as it is: the cumulative sum over the selected
    rows alone, behind a row of zeros, is the same additions.  Nobody selected: A * 0.0.  A NaN value is in no bin and no range."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(len(rows), rows.size // max(len(rows), 1) if len(rows) else (rows.shape[1] if rows.ndim > 1 else 0))
    x = np.asarray(x, dtype=np.float64).ravel()
    A = np.float64(A)
    zero = np.zeros((1, rows.shape[1]))

    def osum(mask):
        return np.cumsum(np.concatenate([zero, rows[mask]]), axis=0)[-1]

    with np.errstate(all='ignore'):
        rng = A * osum((x > lower) & (x < upper))
        if not bins:
            return rng, None
        e = np.asarray(edges, dtype=np.float64).ravel()
        out = np.zeros((max(len(e) - 1, 0), rows.shape[1]))
        for b in range(len(e) - 1):
            out[b] = A * osum((x >= e[b]) & (x < e[b + 1]) & (x < e[-1]))
    return rng, out


class Moments(object):
    """utils/parameter.py:20-154.  `intensity`: the partial intensity of the value range, (mean[nq], std[nq]) over the repetitions
    (:124-154), where the histogram asks for it (Histogram(partialIntensity=...)); None otherwise."""
    intensity = None

    @staticmethod
    def fieldNames():
        return ("totalValue", "totalValueStd", "mean", "meanStd", "variance", "varianceStd",
                "skew", "skewStd", "kurtosis", "kurtosisStd")

    def __init__(self, contribs, paramIndex, valueRange, fraction):
        numReps = contribs.shape[2]
        # (repetition-major copies: the ordered sums below then run along contiguous rows)
        vals = np.ascontiguousarray(contribs[:, paramIndex, :].T)
        fraction = np.ascontiguousarray(np.asarray(fraction).T)
        lo, hi = min(valueRange), max(valueRange)
        # All repetitions at once.  The reference sums the valid contributions of a repetition with the builtin sum(), i.e. in
        # contribution order; a cumulative sum down the contribution axis with the invalid entries replaced by +0.0 adds the
        # same numbers in the same order (x + 0.0 == x bit for bit).  The powers are products (d*d*d, (d*d)*(d*d)): numpy's
        # `**3` / `**4` go through pow(), whose last bit differs between its scalar and its SIMD array path on one machine already
        # (and 40 000 calls of it were most of histogram()'s time); the moments are compared at 1e-6.
        valid = (vals > lo) & (vals < hi)
        anyv = valid.any(axis=1)

        def ssum(x):
            return np.cumsum(np.where(valid, x, 0.0), axis=1)[:, -1] if x.shape[1] else np.zeros(numReps)

        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            tot = ssum(fraction)
            mu = ssum(vals * fraction)
            mu = np.where(tot != 0, mu / np.where(tot != 0, tot, 1.0), mu)
            dev = vals - mu[:, None]
            dev2 = dev * dev
            var = ssum(dev2 * fraction) / tot
            sigma = np.sqrt(np.abs(var))
            # (utils/parameter.py:106-107 skips only an exact zero: a NaN product — all-zero weighting, e.g. 'surf' on a model
            # without surface() — goes on and gives NaN skew / kurtosis, like the variance)
            ok = anyv & ((tot * sigma) != 0.0)
            sigma2 = sigma * sigma
            skw = np.where(ok, ssum(dev2 * dev * fraction) / (tot * (sigma2 * sigma)), 0.0)
            krt = np.where(ok, ssum(dev2 * dev2 * fraction) / (tot * (sigma2 * sigma2)), 0.0)
        val = np.where(anyv, tot, 0.0); mu = np.where(anyv, mu, 0.0); var = np.where(anyv, var, 0.0)
        ddof = 1 if numReps > 1 else 0
        self.total = (val.mean(), val.std(ddof=ddof)); self.mean = (mu.mean(), mu.std(ddof=ddof))
        self.variance = (var.mean(), var.std(ddof=ddof)); self.skew = (skw.mean(), skw.std(ddof=ddof))
        self.kurtosis = (krt.mean(), krt.std(ddof=ddof))

    @classmethod
    def fromRepetitions(cls, val, mu, var, skw, krt):
        """The per-repetition moments worked out elsewhere (mcsas_hip_histogram) -> their mean / std over the repetitions."""
        self = cls.__new__(cls)
        ddof = 1 if len(val) > 1 else 0
        self.total = (val.mean(), val.std(ddof=ddof)); self.mean = (mu.mean(), mu.std(ddof=ddof))
        self.variance = (var.mean(), var.std(ddof=ddof)); self.skew = (skw.mean(), skw.std(ddof=ddof))
        self.kurtosis = (krt.mean(), krt.std(ddof=ddof))
        return self

    @property
    def fields(self):
        return self.total + self.mean + self.variance + self.skew + self.kurtosis


class Histogram(object):
    """utils/parameter.py:187-538: bins, CDF, observability and moments of one parameter."""

    PARTIAL = (None, "range", "bins")

    def __init__(self, param, lower, upper, binCount=50, xscale=None, yweight=None, autoFollow=True, partialIntensity=None):
        """partialIntensity: None, "range" (the scattering curve of the contributions inside the value range: .intensity,
        .moments.intensity) or "bins" (that, and the curve of every bin: .binIntensity); McSAS.histogram() fills them."""
        if partialIntensity not in self.PARTIAL:
            raise ValueError("Histogram: partialIntensity %r (None, 'range' or 'bins')" % (partialIntensity,))
        self.partialIntensity = partialIntensity
        self.intensity = self.binIntensity = None
        self.param = param
        self.binCount = max(0, int(binCount))
        self.xrange = (float(lower), float(upper))
        self.xscale = xscale
        self.yweight = yweight
        self.autoFollow = bool(autoFollow)
        self.xLowerEdge = self.xMean = self.xWidth = None
        self.bins = self.cdf = self.observability = self.moments = None

    @staticmethod
    def xscaling():
        return ('lin', 'log')

    @staticmethod
    def yweighting():
        return ('vol', 'num', 'int', 'surf')

    @property
    def xscale(self):
        return self._xscale

    @xscale.setter
    def xscale(self, kind):                                   # :244-249 (invalid -> 'log')
        kind = str(kind).strip()
        self._xscale = kind if kind in self.xscaling() else 'log'

    @property
    def yweight(self):
        return self._yweight

    @yweight.setter
    def yweight(self, kind):                                  # :255-259 (invalid -> 'vol')
        kind = str(kind).strip()
        self._yweight = kind if kind in self.yweighting() else 'vol'

    @property
    def xrange(self):
        return self._xrange

    @xrange.setter
    def xrange(self, valueRange):                             # :265-270
        lo, hi = min(valueRange), max(valueRange)
        lo, hi = max(self.param.min(), lo), min(self.param.max(), hi)
        self._xrange = (lo, hi)

    @property
    def lower(self):
        return self._xrange[0]

    @property
    def upper(self):
        return self._xrange[1]

    def updateRange(self):                                    # :292-297
        if self.autoFollow:
            self.xrange = self.param.activeRange()
        self.xrange = self.xrange

    def _setXLowerEdge(self):                                 # :349-362
        if 'lin' in self.xscale:
            self.xLowerEdge = np.linspace(self.lower, self.upper, self.binCount + 1)
        else:
            self.xLowerEdge = np.logspace(np.log10(self.lower), np.log10(self.upper), self.binCount + 1)
        self.xWidth = np.diff(self.xLowerEdge)
        self.xMean = (self.xLowerEdge[:-1] + self.xLowerEdge[1:]) / 2.0     # (numpy's mean of two: their sum over 2)

    def calc(self, contribs, paramIndex, fractions):          # :420-439
        self._setXLowerEdge()
        numContribs, dummy, numReps = contribs.shape
        frac, minReq = fractions[self.yweight]
        # _calcBins/_calcBin (:441-469) for every (bin, repetition) at once.  A contribution with
        # edge[b] <= x < edge[b+1] belongs to bin b; numpy.bincount walks its input once, in order, adding weight i to cell
        # index[i] — with the (contribution, repetition) array flattened row-major a cell's members are added in contribution
        # order, the order of the reference's builtin sum() over the masked contributions.
        nb = self.binCount
        par = np.ascontiguousarray(contribs[:, paramIndex, :])
        b = np.searchsorted(self.xLowerEdge, par.ravel(), side='right').reshape(par.shape) - 1
        inb = (b >= 0) & (b < nb) & (par < self.xLowerEdge[-1])
        cell = (b * numReps + np.arange(numReps)[None, :])[inb]
        ncell = nb * numReps
        bins = np.bincount(cell, weights=frac[inb], minlength=ncell)[:ncell].reshape(nb, numReps)
        obsSum = np.bincount(cell, weights=minReq[inb], minlength=ncell)[:ncell].reshape(nb, numReps)
        cnt = np.bincount(cell, minlength=ncell)[:ncell].reshape(nb, numReps).astype(float)
        bins[np.isnan(bins)] = 0.
        with np.errstate(invalid='ignore', divide='ignore'):
            allObs = np.where(cnt > 0, obsSum / cnt, 0.)      # mean of the members' visibility limits
        cdf = np.cumsum(bins, axis=0)                         # _calcCDF :471-479
        top = cdf.max(axis=0) if nb else np.zeros(numReps)
        with np.errstate(invalid='ignore', divide='ignore'):
            cdf = np.where(top[None, :] == 0.0, 0., cdf / top[None, :])
        self._setResults(bins, allObs, cdf)
        self.moments = Moments(contribs, paramIndex, self.xrange, frac)
        self.intensity = self.binIntensity = None             # (McSAS.histogram() fills them after this where they are asked for)

    def _setResults(self, bins, allObs, cdf):
        nb, numReps = bins.shape
        self.bins = VectorResult(bins)
        self.cdf = VectorResult(cdf)
        finite = np.where(allObs < np.inf, allObs, -np.inf)   # _setObservability :390-402
        best = finite.max(axis=1) if numReps else np.zeros(nb)
        self.observability = np.where(np.isfinite(best), best, 0.)

    def deviceSpec(self, paramIndex):
        """What mcsas_hip_histogram needs to know about this histogram (engine.histogram_device)."""
        self._setXLowerEdge()
        spec = dict(param_index=paramIndex, yweight=self.yweight, edges=self.xLowerEdge, lower=min(self.xrange), upper=max(self.xrange))
        if self.partialOnDevice():
            spec["partial"] = self.partialIntensity
        return spec

    def partialOnDevice(self, maxBins=256):
        """Whether the device call takes this histogram's partial intensities: asked for, and for the bin curves no more bins than
        engine.HISTOGRAM_PARTIAL_MAX_BINS and edges that are finite and ascend (McSAS.histogram() takes the others in numpy)."""
        if self.partialIntensity != "bins":
            return self.partialIntensity is not None
        if self.xLowerEdge is None:
            self._setXLowerEdge()
        e = np.asarray(self.xLowerEdge, dtype=float)
        return self.binCount <= maxBins and bool(np.isfinite(e).all() and (np.diff(e) >= 0).all())

    def setIntensity(self, rangeCurves, binCurves=None):
        """The partial intensities of every repetition, range [nq][R] and bin [n_bin][nq][R] or None: .intensity (VectorResult),
        .moments.intensity = (mean[nq], std[nq]) with ddof 1 beyond one repetition (utils/parameter.py:150-154), .binIntensity
        (.full, .mean, .std over the repetitions)."""
        rangeCurves = np.array(rangeCurves, dtype=np.float64)
        self.intensity = VectorResult(rangeCurves)
        ddof = 1 if rangeCurves.shape[1] > 1 else 0
        if self.moments is not None:
            self.moments.intensity = (rangeCurves.mean(axis=1), rangeCurves.std(axis=1, ddof=ddof))
        self.binIntensity = CellResult(np.array(binCurves, dtype=np.float64)) if binCurves is not None else None

    def setFromDevice(self, res):
        """bins / obs / cdf / moments of every repetition as mcsas_hip_histogram returns them (engine.histogram_device)."""
        self._setResults(np.array(res["bins"]), np.array(res["obs"]), np.array(res["cdf"]))
        self.moments = Moments.fromRepetitions(*[np.array(x) for x in res["moments"]])
        self.intensity = self.binIntensity = None
        if "intensity" in res:
            self.setIntensity(res["intensity"], res.get("bin_intensity"))


# ------------------------------------------------------------------ joint histogram of two parameters (post-fit; no reference counterpart)
class CellResult(object):
    """VectorResult for [nx][ny][R] cells: mean / std over the repetitions (ddof 1 where there is more than one)."""

    def __init__(self, arr):
        assert arr.ndim == 3
        self.full = arr
        numReps = arr.shape[2]
        self.mean = arr.mean(axis=2) if numReps else np.zeros(arr.shape[:2])
        self.std = arr.std(axis=2, ddof=1 if numReps > 1 else 0) if numReps else np.zeros(arr.shape[:2])


class Moments2D(object):
    """total, the two means, the two variances, the covariance and the correlation of two parameters over the contributions inside
    both value ranges (strictly), per repetition in `.full` [7][R], each as (mean, std) over the repetitions."""

    NAMES = ("total", "meanX", "meanY", "varianceX", "varianceY", "covariance", "correlation")

    @staticmethod
    def perRepetition(x, y, rangeX, rangeY, fraction):
        """[7][R] from x, y, fraction [N][R]: Moments' ordered sums (a cumulative sum down the contributions with +0.0 in place of
        the contributions outside), in mcsas_hip_histogram2d's operation order (include/mcsas_hip.h)."""
        numReps = x.shape[1]
        x, y, f = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).T) for a in (x, y, fraction))
        valid = (x > min(rangeX)) & (x < max(rangeX)) & (y > min(rangeY)) & (y < max(rangeY))
        anyv = valid.any(axis=1)

        def ssum(t):
            return np.cumsum(np.where(valid, t, 0.0), axis=1)[:, -1] if t.shape[1] else np.zeros(numReps)

        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            tot = ssum(f)
            nz = tot != 0
            mx, my = ssum(x * f), ssum(y * f)
            mx = np.where(nz, mx / np.where(nz, tot, 1.0), mx)
            my = np.where(nz, my / np.where(nz, tot, 1.0), my)
            dx, dy = x - mx[:, None], y - my[:, None]
            vxx, vyy, cxy = ssum((dx * dx) * f) / tot, ssum((dy * dy) * f) / tot, ssum((dx * dy) * f) / tot
            den = np.sqrt(np.abs(vxx)) * np.sqrt(np.abs(vyy))
            # (only an exact zero is skipped: a NaN product goes on and gives NaN, like Moments' skew)
            rho = np.where(den != 0.0, cxy / np.where(den != 0.0, den, 1.0), 0.0)
        return np.where(anyv[None, :], np.stack([tot, mx, my, vxx, vyy, cxy, rho]), 0.0)

    def __init__(self, full):
        self.full = np.asarray(full, dtype=np.float64).reshape(7, -1)
        ddof = 1 if self.full.shape[1] > 1 else 0
        for name, row in zip(self.NAMES, self.full):
            setattr(self, name, (row.mean(), row.std(ddof=ddof)))

    @property
    def fields(self):
        return sum((getattr(self, name) for name in self.NAMES), ())


class Histogram2D(object):
    """The joint histogram of two active fit parameters: which values of one go with which of the other.  Per axis the rules are
    Histogram's: a range clipped to the parameter's value range that follows its active range (autoFollow), 'lin' / 'log' edges
    formed as Histogram._setXLowerEdge forms them, a cell [ex[i], ex[i+1]) x [ey[j], ey[j+1]), every sum in contribution order.
    McSAS.histograms2d holds them; McSAS.histogram() fills .bins (.full [nx][ny][R], .mean, .std), .obs [nx][ny][R] (a cell's mean
    visibility limit per repetition), .observability [nx][ny] and .moments (Moments2D)."""

    def __init__(self, paramX, paramY, rangeX, rangeY, binCount=(20, 20), scaleX='log', scaleY='log', yweight='vol', autoFollow=True):
        self.paramX, self.paramY = paramX, paramY
        nx, ny = (binCount, binCount) if np.isscalar(binCount) else binCount
        self.binCount = (max(0, int(nx)), max(0, int(ny)))
        self.xrange, self.yrange = rangeX, rangeY
        self.scaleX, self.scaleY = scaleX, scaleY
        self.yweight = yweight
        self.autoFollow = bool(autoFollow)
        self.xLowerEdge = self.yLowerEdge = None
        self.bins = self.obs = self.observability = self.moments = None
        for p in (paramX, paramY):                           # (FitParameter.setActiveRange tells its joint histograms too)
            followers = getattr(p, "_histograms2d", None)
            if followers is not None and self not in followers:
                followers.append(self)

    @staticmethod
    def _scale(kind):                                         # (invalid -> 'log', as Histogram.xscale)
        kind = str(kind).strip()
        return kind if kind in Histogram.xscaling() else 'log'

    @staticmethod
    def _clipped(param, valueRange):                          # (as Histogram.xrange)
        lo, hi = min(valueRange), max(valueRange)
        return (max(param.min(), lo), min(param.max(), hi))

    scaleX = property(lambda self: self._scaleX, lambda self, kind: setattr(self, "_scaleX", self._scale(kind)))
    scaleY = property(lambda self: self._scaleY, lambda self, kind: setattr(self, "_scaleY", self._scale(kind)))
    xrange = property(lambda self: self._xrange, lambda self, r: setattr(self, "_xrange", self._clipped(self.paramX, r)))
    yrange = property(lambda self: self._yrange, lambda self, r: setattr(self, "_yrange", self._clipped(self.paramY, r)))

    @property
    def yweight(self):
        return self._yweight

    @yweight.setter
    def yweight(self, kind):                                  # (invalid -> 'vol', as Histogram.yweight)
        kind = str(kind).strip()
        self._yweight = kind if kind in Histogram.yweighting() else 'vol'

    def updateRange(self):                                    # (as Histogram.updateRange, per axis)
        if self.autoFollow:
            self.xrange, self.yrange = self.paramX.activeRange(), self.paramY.activeRange()
        self.xrange, self.yrange = self.xrange, self.yrange

    @staticmethod
    def _edges(valueRange, scale, count):                     # Histogram._setXLowerEdge's expressions
        lower, upper = valueRange
        if 'lin' in scale:
            return np.linspace(lower, upper, count + 1)
        return np.logspace(np.log10(lower), np.log10(upper), count + 1)

    def _setEdges(self):
        self.xLowerEdge = self._edges(self.xrange, self.scaleX, self.binCount[0])
        self.yLowerEdge = self._edges(self.yrange, self.scaleY, self.binCount[1])

    def calc(self, contribs, ix, iy, fractions):
        """The numpy form of mcsas_hip_histogram2d (include/mcsas_hip.h), by Histogram.calc's method: the column of a value is
        searchsorted(side='right') - 1, and numpy.bincount over the row-major flattened (contribution, repetition) array adds a
        cell's members in contribution order.  The path for more contributions or cells than the device call takes."""
        self._setEdges()
        numContribs, dummy, numReps = contribs.shape
        frac, minReq = fractions[self.yweight]
        frac, minReq = np.asarray(frac, dtype=np.float64), np.asarray(minReq, dtype=np.float64)
        nx, ny = self.binCount
        x, y = np.ascontiguousarray(contribs[:, ix, :]), np.ascontiguousarray(contribs[:, iy, :])
        bx = np.searchsorted(self.xLowerEdge, x.ravel(), side='right').reshape(x.shape) - 1
        by = np.searchsorted(self.yLowerEdge, y.ravel(), side='right').reshape(y.shape) - 1
        inb = (bx >= 0) & (bx < nx) & (by >= 0) & (by < ny)
        cell = ((bx * ny + by) * numReps + np.arange(numReps)[None, :])[inb]
        ncell = nx * ny * numReps
        bins = np.bincount(cell, weights=frac[inb], minlength=ncell)[:ncell].reshape(nx, ny, numReps)
        obsSum = np.bincount(cell, weights=minReq[inb], minlength=ncell)[:ncell].reshape(nx, ny, numReps)
        cnt = np.bincount(cell, minlength=ncell)[:ncell].reshape(nx, ny, numReps).astype(float)
        bins[np.isnan(bins)] = 0.
        with np.errstate(invalid='ignore', divide='ignore'):
            allObs = np.where(cnt > 0, obsSum / np.where(cnt > 0, cnt, 1.), 0.)
        self._setResults(bins, allObs, Moments2D.perRepetition(x, y, self.xrange, self.yrange, frac))

    def _setResults(self, bins, allObs, moments):
        self.bins = CellResult(bins)
        self.obs = allObs
        finite = np.where(allObs < np.inf, allObs, -np.inf)   # Histogram._setResults' rule: the largest finite limit, 0 where none
        best = finite.max(axis=2) if allObs.shape[2] else np.zeros(allObs.shape[:2])
        self.observability = np.where(np.isfinite(best), best, 0.)
        self.moments = Moments2D(moments)

    def deviceSpec(self, ix, iy):
        """What mcsas_hip_histogram2d needs to know about this histogram (engine.histogram2d_device)."""
        self._setEdges()
        return dict(param_x=ix, param_y=iy, yweight=self.yweight, edges_x=self.xLowerEdge, edges_y=self.yLowerEdge,
                    lower_x=min(self.xrange), upper_x=max(self.xrange), lower_y=min(self.yrange), upper_y=max(self.yrange))

    def setFromDevice(self, res):
        """bins / obs / moments of every repetition as mcsas_hip_histogram2d returns them (engine.histogram2d_device)."""
        self._setEdges()
        self._setResults(np.array(res["bins"]), np.array(res["obs"]), np.array(res["moments"]))
