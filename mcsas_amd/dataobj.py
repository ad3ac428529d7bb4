"""SASData: the three vectors the hot path reads, under the attribute names the reference uses
(dataobj/sasdata.py:51-75, dataobj/datavector.py:46-116).  File parsing, unit conversion, masking
and log-rebinning stay with the reference front-end (out of scope); `fromCsv` only
covers the plain `q; I; sigma` text layout of testdata/quickstartdemo1.csv for demos and tests.

Beam-profile smearing is configured here exactly as in the reference
(`data.config.smearing`, dataobj/sasconfig.py:17-339): this module only prepares the integration
offsets, profile weights and evaluation points `data.locs`; the smeared intensities themselves are
evaluated by the HIP kernels (include/mcsas_hip.h, smear_* fields)."""
from __future__ import annotations

import numpy as np


class DataVector(object):
    def __init__(self, name, data, dataU=None):
        self.name = name
        self.binnedData = np.asarray(data, dtype=float)
        self.binnedDataU = None if dataU is None else np.asarray(dataU, dtype=float)
        self.sanitized = self.binnedData
        self.limit = [float(self.binnedData.min()), float(self.binnedData.max())] if len(self.binnedData) else [0., 0.]


class _Value(object):
    """Configuration parameter with the reference's accessors (`p()`, `p.value()`, `p.setValue(v)`,
    `p.setValueRange((lo, hi))`); numbers are clipped into the value range like Parameter.setValue
    (bases/algorithm/parameter.py:405-414)."""

    def __init__(self, name, default, valueRange=None, onUpdate=None):
        self._name, self._value, self._range, self._onUpdate = name, default, valueRange, onUpdate

    def name(self):
        return self._name

    def value(self):
        return self._value

    __call__ = value

    def valueRange(self):
        return self._range

    def max(self):
        return self._range[1]

    def setValueRange(self, rng):
        self._range = (min(rng), max(rng))
        if not isinstance(self._value, bool):
            self._value = type(self._value)(min(max(self._value, self._range[0]), self._range[1]))

    def setValue(self, v):
        if isinstance(self._value, bool):
            self._value = bool(v)
        else:
            if self._range is not None:
                v = min(max(v, self._range[0]), self._range[1])
            self._value = type(self._value)(v)
        if self._onUpdate is not None:
            self._onUpdate()


class SmearingConfig(object):
    """dataobj/sasconfig.py:17-75: common part of the beam-profile descriptions."""

    def __init__(self):
        self.doSmear = _Value("doSmear", False)
        self.nSteps = _Value("nSteps", 25, (0, 1000))
        self.twoDColl = _Value("twoDColl", False)
        self._qOffset = self._weights = None

    @property
    def qOffset(self):
        return self._qOffset

    @property
    def weights(self):
        return self._weights

    @property
    def prepared(self):
        return self._qOffset, self._weights

    def updateSmearingLimits(self, q):
        pass

    def _offsets(self, lo, hi):
        """Integration offsets: `nSteps` log-spaced points plus zero for slit collimation, mirrored
        ceil(nSteps/2) points plus zero for 2-D (pinhole) collimation (sasconfig.py:132-142)."""
        n = int(self.nSteps())
        if self.twoDColl():
            off = np.logspace(np.log10(lo), np.log10(hi), num=int(np.ceil(n / 2.)))
            return np.concatenate((-off[::-1], [0.], off))
        return np.concatenate(([0.], np.logspace(np.log10(lo), np.log10(hi), num=n)))


class TrapezoidSmearing(SmearingConfig):
    """Trapezoidal beam profile with top width `umbra` and bottom width `penumbra`
    (sasconfig.py:77-184)."""

    def __init__(self):
        super(TrapezoidSmearing, self).__init__()
        self.penumbra = _Value("penumbra", 0., (0., np.inf))
        self.umbra = _Value("umbra", 0., (0., np.inf), onUpdate=self.onUmbraUpdate)

    def onUmbraUpdate(self):                                 # :178-182
        self.penumbra.setValueRange((self.umbra(), self.penumbra.max()))

    def inputValid(self):                                    # :94-96
        return (self.umbra() > 0.) and (self.penumbra() > self.umbra())

    @staticmethod
    def halfTrapzPDF(x, c, d):                               # :104-120
        assert d > 0.
        x = np.abs(x)
        pdf = x * 0.
        pdf[x < c] = 1.
        if d > c:
            slope = (c <= x) & (x < d)
            pdf[slope] = (1. / (d - c)) * (d - x[slope])
        norm = 1. / (d + c)
        return pdf * norm, norm

    def setIntPoints(self, q):                               # :122-149
        xt, xb = self.umbra(), self.penumbra()
        off = self._offsets(q.min() / 5., xb / 2.)
        y, _ = self.halfTrapzPDF(off, xt, xb)
        self._qOffset, self._weights = off, y

    def updateSmearingLimits(self, q):                       # :169-173
        low, high = np.absolute(np.diff(q)).min(), q.max()
        self.umbra.setValueRange((low, 2. * high))
        self.penumbra.setValueRange((low, 2. * high))


class GaussianSmearing(SmearingConfig):
    """Gaussian beam profile; the parameter the reference calls `variance` is used as the standard
    deviation of the profile (sasconfig.py:186-260, scipy.stats.norm.pdf(scale=variance))."""

    def __init__(self):
        super(GaussianSmearing, self).__init__()
        self.variance = _Value("variance", 0., (0., np.inf))

    def inputValid(self):                                    # :198-200
        return self.variance() > 0.

    def setIntPoints(self, q):                               # :209-233
        g = self.variance()
        off = self._offsets(q.min() / 3., 2.5 * g)
        self._qOffset = off
        self._weights = np.exp(-0.5 * (off / g) ** 2) / (g * np.sqrt(2. * np.pi))

    def updateSmearingLimits(self, q):                       # :251-256
        low, high = np.absolute(np.diff(q)).min(), q.max()
        self.variance.setValueRange((low, 2. * high))


class SASConfig(object):
    """The part of dataobj/sasconfig.py:262-360 the Monte-Carlo path reads: `smearing`."""

    def __init__(self, smearing=None):
        self.smearing = smearing if smearing is not None else TrapezoidSmearing()

    def prepareSmearing(self, q):                            # :308-339
        q = np.asarray(q, dtype=float)
        assert q.ndim == 1
        sm = self.smearing
        if sm is None or not sm.inputValid() or not sm.doSmear():
            if sm is not None:
                sm._qOffset = sm._weights = None
            return q
        sm.setIntPoints(q)
        qOffset, weights = sm.prepared
        if not sm.twoDColl():                                # slit collimation
            return np.sqrt(np.add.outer(q ** 2, qOffset ** 2))
        return np.add.outer(q, qOffset)                      # azimuthally averaged 2-D pattern


class SmearArgs(object):
    """What the kernels need of a prepared smearing configuration (engine.HipProblem `smear=`)."""

    def __init__(self, locs, q_offset, weights):
        self.locs, self.q_offset, self.weights = locs, q_offset, weights


class SASData(object):
    def __init__(self, q, intensity, sigma, f_limit=None, title="data", config=None):
        self.title = title
        self.x0 = DataVector("q", q)
        self.f = DataVector("I", intensity, sigma)
        if f_limit is not None:          # limits of the UN-binned intensities (datavector.py:52)
            self.f.limit = [float(f_limit[0]), float(f_limit[1])]
        self.config = config if config is not None else SASConfig()
        if self.config.smearing is not None and self.count > 1:
            self.config.smearing.updateSmearingLimits(self.x0.binnedData)
        self.updateConfig()

    def updateConfig(self):              # dataobj/sasdata.py:161-165: call after changing config.smearing
        self.locs = self.config.prepareSmearing(self.x0.binnedData)

    def smearArgs(self, model):
        """-> SmearArgs when calcIntensity would take the smeared branch for `model`
        (bases/model/sasmodel.py:56-60), else None."""
        sm = self.config.smearing
        if (sm is None or not getattr(model, "canSmear", False) or not sm.doSmear() or not sm.inputValid()):
            return None
        self.updateConfig()
        return SmearArgs(self.locs, sm.qOffset, sm.weights)

    @property
    def q(self):
        return self.x0.binnedData

    @property
    def count(self):
        return len(self.x0.binnedData)

    def sphericalSizeEst(self):          # dataobj/sasdata.py:105 (pi / q limits)
        return np.array([np.pi / self.x0.limit[1], np.pi / self.x0.limit[0]])

    @classmethod
    def fromRaw(cls, q, intensity, sigma=None, nBin=100, fuMin=0.01, title="data", device=-1):
        """Raw SI vectors -> the data object McSAS.analyse reads, the way DataObj prepares it
        (dataobj/dataobj.py): uncertainty floor fuMin*I (_prepareUncertainty, :204-227), points with
        q <= 0 or non-finite entries dropped (the default masks, :239-263), then log-spaced rebinning into
        at most nBin bins (_reBin, :288-345; nBin = 0: none).  Both steps run on the GPU
        (mcsas_hip_prepare_uncertainty, mcsas_hip_rebin)."""
        from . import engine
        q, intensity = np.asarray(q, dtype=float), np.asarray(intensity, dtype=float)
        su = engine.prepare_uncertainty(intensity, sigma, fuMin, device=device)
        ok = np.isfinite(q) & (q > 0.) & np.isfinite(intensity)
        qs, fs, us = q[ok], intensity[ok], su[ok]
        f_limit = [float(fs.min()), float(fs.max())]         # limits of the un-binned intensities (datavector.py:52)
        if nBin and nBin > 0:
            qs, fs, us = engine.rebin(qs, fs, us, int(nBin), device=device)
        return cls(qs, fs, us, f_limit=f_limit, title=title)

    @classmethod
    def fromCsv(cls, filename, q_unit=1e9):
        raw = open(filename, "rb").read().decode("utf-8", "replace").replace("\r", "\n")
        rows = []
        for line in raw.split("\n"):
            parts = [x for x in line.replace(";", " ").replace(",", " ").split() if x]
            try:
                rows.append([float(x) for x in parts[:3]])
            except ValueError:
                continue
        arr = np.array([r for r in rows if len(r) == 3])
        return cls(arr[:, 0] * q_unit, arr[:, 1], arr[:, 2], title=filename)


class DataSets(object):
    """Several measurements of ONE specimen — two detector distances, SAXS + WAXS, two instruments — for a joint fit: wraps the
    members' SASData objects.  With `algo.data = DataSets([d0, d1, ...])` McSAS.analyse() fits one population to all members at once,
    each with a least-squares scale and background of its own at every step (engine.analyse_sets; include/mcsas_hip.h:
    mcsas_hip_analyse_sets_mode); 1 to engine.MAX_SETS members of at least 3 points each.  The vectors the fit reads (`q`,
    `f.binnedData`, `f.binnedDataU`, `x0`) are the members' one after the other, and `slices` says where each member lies in them.
    `sharedScale` (default False): the members are on an absolute scale — ONE least-squares scale for all of them, a background per
    member, and so one volume fraction per contribution.  A known relative scale k_s between the members is the caller's: divide
    that member's intensity and uncertainty by it before wrapping it here.
    `histogramSet` (default 0): whose points judge what is visible in histogram() — a member's index or "all".  With an index and
    sharedScale=False histogram() and the partial histograms take the existing single-set path with that member's data alone, whose
    scale fit is exactly the joint fit's for that member, so fractions are consistent with it — and the visibility limits are those
    "as seen by that set": a size another member would see and this one does not counts as invisible.  With "all" (or with
    sharedScale=True) histogram() runs over the points of all members (engine.histogram_sets): every member is fitted to the summed
    intensity as the joint fit does, a contribution is visible where ANY named member's points show it, and volume fractions are by
    member `scaleSet`'s scale (default 0; with sharedScale the shared scale).  That path offers no partial intensities
    (Histogram(partialIntensity=...) raises ValueError).  Smearing configurations of the members are not used (the joint fit refuses
    smearing)."""

    def __init__(self, members, histogramSet=0, title="data sets", sharedScale=False, scaleSet=0):
        self.members = list(members)
        if not self.members:
            raise ValueError("DataSets: needs at least one SASData")
        for d in self.members:
            if not (hasattr(d, "x0") and hasattr(d, "f")) or d.f.binnedDataU is None:
                raise ValueError("DataSets: every member is a SASData with q, intensity and sigma")
        self.title = title
        if isinstance(histogramSet, str):
            if histogramSet != "all":
                raise ValueError("DataSets.histogramSet %r: a member's index or \"all\"" % (histogramSet,))
            self.histogramSet = "all"
        else:
            self.histogramSet = int(histogramSet)
        self.sharedScale = bool(sharedScale)
        self.scaleSet = int(scaleSet)
        if not 0 <= self.scaleSet < len(self.members):
            raise ValueError("DataSets.scaleSet %d: there are %d members" % (self.scaleSet, len(self.members)))
        self.x0 = DataVector("q", np.concatenate([d.x0.binnedData for d in self.members]))
        self.f = DataVector("I", np.concatenate([d.f.binnedData for d in self.members]),
                            np.concatenate([d.f.binnedDataU for d in self.members]))
        self.f.limit = [min(d.f.limit[0] for d in self.members), max(d.f.limit[1] for d in self.members)]
        edges = np.concatenate([[0], np.cumsum([d.count for d in self.members])])
        self.slices = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]

    def __len__(self):
        return len(self.members)

    def jointHistogram(self):
        """histogram() runs over the points of all members (engine.histogram_sets), not against one member alone"""
        return self.sharedScale or self.histogramSet == "all"

    def visibleSets(self):
        """the members whose points judge what is visible"""
        if self.histogramSet == "all":
            return list(range(len(self.members)))
        self.histogramMember()
        return [self.histogramSet]

    def histogramMember(self):
        if self.histogramSet == "all":
            raise ValueError("DataSets.histogramSet \"all\": the histogram is judged by all members, not by one")
        if not 0 <= self.histogramSet < len(self.members):
            raise ValueError("DataSets.histogramSet %d: there are %d members" % (self.histogramSet, len(self.members)))
        return self.members[self.histogramSet]

    def triples(self):
        """[(q, I, sigma)] of the members: engine.analyse_sets' `sets`"""
        return [(d.x0.binnedData, d.f.binnedData, d.f.binnedDataU) for d in self.members]

    def smearArgs(self, model):
        return None

    @property
    def q(self):
        return self.x0.binnedData

    @property
    def count(self):
        return len(self.x0.binnedData)

    def sphericalSizeEst(self):
        return np.array([np.pi / self.x0.limit[1], np.pi / self.x0.limit[0]])
