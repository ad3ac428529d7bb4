#!/usr/bin/env python3
"""Golden-vector generator: runs the REAL reference (read-only at /root/reference) in this
container and stores inputs + expected outputs as small fixtures under tests/golden/.

TEST INFRASTRUCTURE ONLY.  Never imported by the product (mcsas_amd/) and never run on the GPU
box (the reference does not travel).  Re-run here with:

    python3 oracle/make_golden.py            # writes tests/golden/*.npz

It needs three throw-away stand-ins for third-party modules that are missing in this image
(`future`, `QtWidgets`).  They hold no McSAS logic and are written to
a temp dir outside the repo by `_install_shims()`.

What is captured, all from the reference's own code paths:
  G1  ScatteringModel.formfactor(q) per model / parameter set     (sphere.py:55, cylindersisotropic.py:50,
      ellipsoidalcoreshell.py:59, kholodenko.py:81)
  G2  ScatteringModel.calc(data, pset, c) -> cumInt, vset, wset, sset  (scatteringmodel.py:79-109)
  G3  BackgroundScalingFit.calc -> sc, conval, aGoFs for 3 flag combos (backgroundscalingfit.py:112-139)
  G4  McSAS.mcFit / McSAS.analyse trajectories with the global numpy RNG seeded, so the consumed
      uniform stream is known (mcsas.py:191-439)
  G5  McSAS.histogram -> Histogram bins/cdf/observability/moments     (mcsas.py:445-615, utils/parameter.py)
  G6  generateParameters transforms (uniform / exponential)            (scatteringmodel.py:117-127)
  G7  beam-profile smearing: SmearingConfig.setIntPoints, SASConfig.prepareSmearing, the smeared branch of
      SASModel.calcIntensity and one mcFit chain on it (dataobj/sasconfig.py:17-339, sasmodel.py:56-73);
      needs numpy.logspace's pre-1.18 float->int truncation, see _LogspaceCompat
  G8  input preparation: DataObj._prepareUncertainty and DataObj._reBin (dataobj/dataobj.py:204-227,288-345)
"""
import os, sys, tempfile, logging, re

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def _install_shims():
    d = tempfile.mkdtemp(prefix="mcsas_shim_")
    os.makedirs(os.path.join(d, "future"))
    open(os.path.join(d, "future", "__init__.py"), "w").close()
    with open(os.path.join(d, "future", "standard_library.py"), "w") as f:
        f.write("def install_aliases(): pass\n")
    with open(os.path.join(d, "future", "utils.py"), "w") as f:
        f.write(
            "def with_metaclass(meta, *bases):\n"
            "    class metaclass(type):\n"
            "        def __new__(cls, name, this_bases, d): return meta(name, bases, d)\n"
            "        @classmethod\n"
            "        def __prepare__(cls, name, this_bases): return meta.__prepare__(name, bases)\n"
            "    return type.__new__(metaclass, 'temporary_class', (), {})\n")
    with open(os.path.join(d, "QtWidgets.py"), "w") as f:
        f.write(
            "class QApplication(object):\n"
            "    @staticmethod\n"
            "    def processEvents(): pass\n"
            "    @staticmethod\n"
            "    def translate(ctx, s): return s\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [d, REF]


_install_shims()
import numpy as np                                            # noqa: E402
from mcsas.datafile import loaddatafile                       # noqa: E402
from mcsas.dataobj.sasdata import SASData                     # noqa: E402
from mcsas.mcsas import McSAS                                 # noqa: E402
from mcsas.mcsas.backgroundscalingfit import BackgroundScalingFit  # noqa: E402
from mcsas.models.sphere import Sphere                        # noqa: E402
from mcsas.models.cylindersisotropic import CylindersIsotropic    # noqa: E402
from mcsas.models.ellipsoidalcoreshell import EllipsoidalCoreShell  # noqa: E402
from mcsas.models.kholodenko import Kholodenko                # noqa: E402
from mcsas.models.ellipsoidsisotropic import EllipsoidsIsotropic   # noqa: E402
from mcsas.models.sphericalcoreshell import SphericalCoreShell      # noqa: E402
from mcsas.models.gaussianchain import GaussianChain          # noqa: E402
from mcsas.models.lmadensesphere import LMADenseSphere        # noqa: E402
from mcsas.utils.parameter import Histogram                   # noqa: E402
from mcsas.bases.algorithm.numbergenerator import (RandomUniform, RandomExponential,   # noqa: E402
                                   RandomExponential2, RandomExponential3)


# ---------------------------------------------------------------- helpers
class AcceptCapture(logging.Handler):
    """mcFit logs one INFO line per accepted move ("... good iter {it}: ...", mcsas.py:385)."""
    rx = re.compile(r"good iter (\d+):")

    def __init__(self):
        super().__init__(level=logging.INFO)
        self.iters = []

    def emit(self, record):
        m = self.rx.search(record.getMessage())
        if m:
            self.iters.append(int(m.group(1)))


def quiet_logging(capture=None):
    root = logging.getLogger()
    for h in list(root.handlers):
        root.removeHandler(h)
    root.setLevel(logging.INFO)
    root.addHandler(logging.NullHandler())
    if capture is not None:
        root.addHandler(capture)


class QOnly(object):
    """formfactor() only needs `.q` (sasmodel.py:26-35 getQ / models use dataset.q)."""
    def __init__(self, q):
        self.q = q


def sasdata(q_nm, I, sigma, nbin=0):
    raw = np.stack([q_nm, I, sigma], axis=1)
    d = SASData(title="syn", rawArray=raw)
    d.config.nBin.setValue(nbin)
    d._reBin()          # dataobj.py:288: nBin == 0 leaves the sanitized vectors un-binned
    return d


def data_vectors(d):
    sig = np.array(d.f.binnedDataU, dtype=float)
    return dict(q=np.array(d.q, dtype=float), I=np.array(d.f.binnedData, dtype=float),
                sigma=sig, f_limit=np.array(d.f.limit, dtype=float),
                x0_limit=np.array(d.x0.limit, dtype=float))


def fix_intdiv(m):
    # cylindersisotropic.py:37 float default breaks numpy.linspace on numpy>=2 (SURVEY §8c gotcha 5)
    m.intDiv.setValue(101)
    m.intDiv.setValue(100)


def new_algo(**kw):
    algo = McSAS.factory()()
    algo.stop = False
    for k, v in kw.items():
        getattr(algo, k).setValue(v)
    return algo


def synthetic_sphere_data(Q, seed=20250101, qmin=0.01, qmax=3.0):
    """tri-modal sphere population, 1 % uncertainty + noise, flat background 0."""
    q_nm = np.logspace(np.log10(qmin), np.log10(qmax), Q)
    rs = np.random.RandomState(seed)
    radii = np.concatenate([rs.normal(8, 3, 300), rs.normal(40, 10, 150), rs.normal(100, 10, 50)])
    radii = np.abs(radii) + 0.5
    I = np.zeros(Q)
    for R in radii:
        x = q_nm * R
        F = 3 * (np.sin(x) - x * np.cos(x)) / x**3
        I += (4 * np.pi / 3 * R**3)**2 * F**2
    I *= 1e-3 / I.max() * 1e6
    sigma = 0.01 * I
    I = I + sigma * rs.normal(size=Q)
    return q_nm, I, sigma


# ---------------------------------------------------------------- G1 / G2 / G6
def model_cases():
    cases = []
    # (tag, model factory, active names, generator-kind overrides, param sets (SI))
    def sph():
        return Sphere()
    cases.append(("sphere", sph, ["radius"],
                  [[1e-9], [3.2e-9], [1.0e-8], [5.0e-8], [3.14e-7], [7.77e-10]]))

    def cyl_aspect():
        m = CylindersIsotropic(); fix_intdiv(m)
        m.radius.setActive(True); m.aspect.setActive(True)
        return m
    cases.append(("cyl_aspect", cyl_aspect, ["radius", "aspect"],
                  [[1e-9, 10.0], [5e-9, 0.3], [2.5e-8, 2.0], [1e-7, 1.0], [3e-10, 50.0]]))

    def cyl_length():
        m = CylindersIsotropic(); fix_intdiv(m)
        m.useAspect.setValue(False)
        m.radius.setActive(True); m.length.setActive(True)
        return m
    cases.append(("cyl_length", cyl_length, ["radius", "length"],
                  [[1e-9, 1e-8], [5e-9, 2e-7], [4e-8, 1e-8]]))

    def ell():
        m = EllipsoidalCoreShell()
        m.a.setActive(True); m.b.setActive(True); m.t.setActive(True)
        return m
    cases.append(("ellcs", ell, ["a", "b", "t"],
                  [[1e-9, 1e-8, 1e-9], [1e-8, 1.5e-8, 5e-8], [1e-7, 2e-9, 1e-10], [2e-10, 3e-7, 4e-9]]))

    def kho():
        return Kholodenko()
    cases.append(("kholodenko", kho, ["radius", "lenKuhn", "lenContour"],
                  [[1e-9, 1e-8, 1e-6], [3e-9, 3e-8, 2.5e-7], [5e-9, 5e-8, 1e-7], [1.2e-9, 1.0e-8, 9.9e-7]]))
    def elliso():
        m = EllipsoidsIsotropic()
        m.a.setActive(True); m.aspect.setActive(True)
        return m
    cases.append(("elliso", elliso, ["a", "aspect"],
                  [[1e-9, 10.0], [5e-9, 0.3], [2.5e-8, 2.0], [1e-7, 1.0]]))

    def sphcs():
        m = SphericalCoreShell()
        m.radius.setActive(True); m.t.setActive(True)
        return m
    cases.append(("sphcs", sphcs, ["radius", "t"],
                  [[1e-9, 1e-9], [1e-8, 5e-9], [1e-7, 2e-10], [3e-9, 3e-8]]))

    def gchain():
        m = GaussianChain()
        m.rg.setActive(True); m.bp.setActive(True)
        return m
    cases.append(("gausschain", gchain, ["rg", "bp"],
                  [[1e-9, 1e-7], [1e-8, 5e-8], [6e-8, 3e-7], [2.5e-9, 1e-9]]))

    def lma():
        m = LMADenseSphere()
        m.radius.setActive(True); m.volFrac.setActive(True)
        return m
    cases.append(("lmasphere", lma, ["radius", "volFrac"],
                  [[1e-9, 0.1], [1e-8, 0.3], [8e-8, 0.02], [3e-9, 0.45]]))
    return cases


def gen_model_vectors():
    out = {}
    q = np.logspace(7, np.log10(3e9), 48)
    qk = np.concatenate([np.logspace(7, np.log10(3e9), 14), [3.0 / 3e-8, 3.0 / 1e-8]])  # incl. q == 3/l_k
    cexp = 0.6666666
    for tag, factory, names, psets in model_cases():
        m = factory()
        qq = qk if tag == "kholodenko" else q
        # model.calc needs a data object with f.binnedData for shape (scatteringmodel.py:89);
        # use ITS q everywhere (unit round trip nm^-1 -> SI is not exact to the last bit)
        d = sasdata(qq * 1e-9, np.ones_like(qq), 0.01 * np.ones_like(qq))
        qq = np.array(d.q, dtype=float)
        ds = QOnly(qq)
        ff = []
        for pv in psets:
            for n, v in zip(names, pv):
                getattr(m, n).setValue(v)
            ff.append(np.array(m.formfactor(ds), dtype=float))
        out[tag + "_q"] = qq
        out[tag + "_pset"] = np.array(psets, dtype=float)
        out[tag + "_ff"] = np.array(ff)
        md = m.calc(d, np.array(psets, dtype=float), cexp)
        out[tag + "_cumInt"] = np.array(md.cumInt)
        out[tag + "_vset"] = np.array(md.vset)
        out[tag + "_wset"] = np.array(md.wset)
        out[tag + "_sset"] = np.array(md.sset)
        # per-row intensities via single-row calc
        rows = []
        for pv in psets:
            rows.append(np.array(m.calc(d, np.array([pv], dtype=float), cexp).cumInt))
        out[tag + "_rows"] = np.array(rows)
    out["comp_exp"] = cexp
    np.savez_compressed(os.path.join(OUT, "g12_models.npz"), **out)
    print("G1/G2 written")


def gen_generators():
    """G6: value transforms for a known uniform stream."""
    out = {}
    seed = 424242
    u = np.random.RandomState(seed).random_sample(64)
    out["u"] = u
    for name, G in (("uniform", RandomUniform), ("exp1", RandomExponential),
                    ("exp2", RandomExponential2), ("exp3", RandomExponential3)):
        np.random.seed(seed)
        out[name] = np.array(G.get(64), dtype=float)
    # scaled through a FitParameter (activeRange ∩ valueRange)
    m = CylindersIsotropic(); fix_intdiv(m)
    m.radius.setActive(True); m.aspect.setActive(True)
    m.radius.setActiveRange((2e-9, 8e-8)); m.aspect.setActiveRange((0.5, 20.0))
    np.random.seed(seed)
    out["cyl_params"] = np.array(m.generateParameters(32), dtype=float)   # column-major draw order
    out["cyl_lo"] = np.array([min(m.radius.activeRange()), min(m.aspect.activeRange())])
    out["cyl_hi"] = np.array([max(m.radius.activeRange()), max(m.aspect.activeRange())])
    s = Sphere(); s.radius.setActiveRange((1e-9, 3e-7))
    np.random.seed(seed)
    out["sph_params"] = np.array(s.generateParameters(64), dtype=float)
    out["sph_lo"] = np.array([1e-9]); out["sph_hi"] = np.array([3e-7])
    np.savez_compressed(os.path.join(OUT, "g6_generators.npz"), **out)
    print("G6 written")


# ---------------------------------------------------------------- G3
def gen_bgfit():
    out = {}
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    dv = data_vectors(d)
    out.update({"q": dv["q"], "I": dv["I"], "sigma": dv["sigma"]})
    m = Sphere()
    rs = np.random.RandomState(7)
    cases = []
    for ci in range(4):
        pset = rs.uniform(3e-9, 3e-7, size=(60, 1))
        md = m.calc(d, pset, 0.6666666)
        C = np.array(md.cumInt)
        sc0 = np.array([dv["f_limit"][1] / C.max(), dv["f_limit"][0]])
        for fb, pb in ((True, False), (False, False), (True, True)):
            bg = BackgroundScalingFit(fb, pb, m)
            sc1, cv1, _, ag1 = bg.calc(d, md, sc0.copy(), ver=1)
            sc2, cv2, _, ag2 = bg.calc(d, md, np.array(sc1, dtype=float).copy())
            cases.append((ci, fb, pb, C, sc0, np.array(sc1), cv1, ag1, np.array(sc2), cv2, ag2))
    # a case that forces a negative background so positiveBackground matters
    Ineg = dv["I"] - 3.0 * dv["I"].min()
    d2 = sasdata(dv["q"] * 1e-9, Ineg, dv["sigma"])
    pset = rs.uniform(3e-9, 3e-7, size=(60, 1))
    md = m.calc(d2, pset, 0.6666666)
    C = np.array(md.cumInt)
    sc0 = np.array([d2.f.limit[1] / C.max(), d2.f.limit[0]])
    out["neg_I"] = np.array(d2.f.binnedData); out["neg_sigma"] = np.array(d2.f.binnedDataU)
    out["neg_C"] = C; out["neg_sc0"] = sc0
    for fb, pb, key in ((True, False, "neg_free"), (True, True, "neg_pos")):
        bg = BackgroundScalingFit(fb, pb, m)
        sc1, cv1, _, ag1 = bg.calc(d2, md, sc0.copy(), ver=1)
        sc2, cv2, _, ag2 = bg.calc(d2, md, np.array(sc1, dtype=float).copy())
        out[key] = np.array([sc2[0], sc2[1], cv2, ag2])
    out["C"] = np.array([c[3] for c in cases])
    out["flags"] = np.array([[c[0], c[1], c[2]] for c in cases], dtype=int)
    out["sc0"] = np.array([c[4] for c in cases])
    out["simplex"] = np.array([[c[5][0], c[5][1], c[6], c[7]] for c in cases])
    out["lm"] = np.array([[c[8][0], c[8][1], c[9], c[10]] for c in cases])
    out["num_params"] = 1
    np.savez_compressed(os.path.join(OUT, "g3_bgfit.npz"), **out)
    print("G3 written")


# ---------------------------------------------------------------- G4
def run_mcfit(algo, n, seed):
    cap = AcceptCapture(); quiet_logging(cap)
    np.random.seed(seed)
    rset, fit, conval, details = algo.mcFit(n, outputMeasVal=True, outputDetails=True, nRun=0)
    quiet_logging(None)
    return dict(rset=np.array(rset), fit=np.array(fit), conval=float(conval),
                num_iter=int(details["numIterations"]), num_moves=int(details["numMoves"]),
                scaling=float(details["scaling"]), background=float(details["background"]),
                accepted=np.array(cap.iters, dtype=np.int64), seed=seed)


def save_traj(name, dv, spec, res, extra=None):
    out = {}
    out.update({"data_" + k: v for k, v in dv.items()})
    out.update({"spec_" + k: np.array(v) for k, v in spec.items()})
    out.update({"res_" + k: v for k, v in res.items()})
    n_draw = int(spec["n_contrib"]) * len(spec["lo"]) + res["num_iter"] * len(spec["lo"])
    out["stream"] = np.random.RandomState(res["seed"]).random_sample(n_draw + 8)
    if extra:
        out.update(extra)
    np.savez_compressed(os.path.join(OUT, name), **out)
    print(name, "iters", res["num_iter"], "moves", res["num_moves"], "chisq", res["conval"])


def gen_trajectories():
    # T1: config 1 plumbing case (quickstartdemo1 -> Q=100 after default rebin), fixed 3000 steps
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    dv = data_vectors(d)
    m = Sphere(); m.radius.setActiveRange(tuple(d.sphericalSizeEst()))
    algo = new_algo(numContribs=200, numReps=1, maxIterations=3000, convergenceCriterion=1e-9)
    algo.model = m; algo.data = d
    spec = dict(model="sphere", n_contrib=200, lo=[min(m.radius.activeRange())],
                hi=[max(m.radius.activeRange())], gen=[0], comp_exp=0.6666666, max_iter=3000,
                conv_crit=1e-9, sld=m.sld())
    save_traj("g4_sphere_q100_fixed.npz", dv, spec, run_mcfit(algo, 200, 1001))

    # T2: same data, run to convergence (crit = 1)
    algo = new_algo(numContribs=200, numReps=1, maxIterations=100000, convergenceCriterion=1.0)
    algo.model = m; algo.data = d
    spec.update(max_iter=100000, conv_crit=1.0)
    save_traj("g4_sphere_q100_converge.npz", dv, spec, run_mcfit(algo, 200, 1002))

    # T3: synthetic 512 q x 400 contribs (BASELINE config 2 shape), 1500 fixed steps
    q_nm, I, sig = synthetic_sphere_data(512)
    d3 = sasdata(q_nm, I, sig)
    dv3 = data_vectors(d3)
    assert d3.count == 512
    m3 = Sphere(); m3.radius.setActiveRange((np.pi / dv3["q"].max(), np.pi / dv3["q"].min()))
    algo = new_algo(numContribs=400, numReps=1, maxIterations=1500, convergenceCriterion=1e-9)
    algo.model = m3; algo.data = d3
    spec3 = dict(model="sphere", n_contrib=400, lo=[min(m3.radius.activeRange())],
                 hi=[max(m3.radius.activeRange())], gen=[0], comp_exp=0.6666666, max_iter=1500,
                 conv_crit=1e-9, sld=m3.sld())
    save_traj("g4_sphere_q512_fixed.npz", dv3, spec3, run_mcfit(algo, 400, 1003))

    # T3b: startFromMinimum + no background + positive background variants (short)
    for tag, kw in (("nobg", dict(findBackground=False)), ("posbg", dict(positiveBackground=True)),
                    ("frommin", dict(startFromMinimum=True))):
        algo = new_algo(numContribs=60, numReps=1, maxIterations=400, convergenceCriterion=1e-9, **kw)
        algo.model = m; algo.data = d
        s = dict(spec); s.update(n_contrib=60, max_iter=400, conv_crit=1e-9,
                                 find_bg=int(kw.get("findBackground", True)),
                                 pos_bg=int(kw.get("positiveBackground", False)),
                                 from_min=int(kw.get("startFromMinimum", False)))
        res = run_mcfit(algo, 60, 1010)
        if tag == "frommin":   # no init draws are consumed
            s["n_contrib_draws"] = 0
        save_traj("g4_sphere_q100_%s.npz" % tag, dv, s, res)

    # T4: cylinders (radius + aspect active, exponential generators), small
    q_nm = np.logspace(np.log10(0.02), np.log10(2.0), 40)
    rs = np.random.RandomState(5)
    mc = CylindersIsotropic(); fix_intdiv(mc)
    mc.radius.setActive(True); mc.aspect.setActive(True)
    mc.radius.setActiveRange((1e-9, 5e-8)); mc.aspect.setActiveRange((0.2, 20.0))
    truth = np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(1, 8, 30)], axis=1)
    dtmp = sasdata(q_nm, np.ones(40), 0.01 * np.ones(40))
    It = np.array(mc.calc(dtmp, truth, 0.6666666).cumInt)
    It = It / It.max() * 1e3
    d4 = sasdata(q_nm, It * (1 + 0.01 * rs.normal(size=40)), 0.01 * It)
    dv4 = data_vectors(d4)
    algo = new_algo(numContribs=40, numReps=1, maxIterations=250, convergenceCriterion=1e-9)
    algo.model = mc; algo.data = d4
    spec4 = dict(model="cyl_aspect", n_contrib=40, lo=[1e-9, 0.2], hi=[5e-8, 20.0], gen=[1, 1],
                 comp_exp=0.6666666, max_iter=250, conv_crit=1e-9, sld=mc.sld(), int_div=100)
    save_traj("g4_cyl_q40.npz", dv4, spec4, run_mcfit(algo, 40, 1004))

    # T5: core-shell ellipsoid (a, b, t active)
    me = EllipsoidalCoreShell()
    me.a.setActive(True); me.b.setActive(True); me.t.setActive(True)
    me.a.setActiveRange((1e-9, 5e-8)); me.b.setActiveRange((2e-9, 1e-7)); me.t.setActiveRange((2e-10, 1e-8))
    truth = np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(5e-9, 4e-8, 30), rs.uniform(5e-10, 5e-9, 30)], axis=1)
    It = np.array(me.calc(dtmp, truth, 0.6666666).cumInt)
    It = It / It.max() * 1e3
    d5 = sasdata(q_nm, It * (1 + 0.01 * rs.normal(size=40)), 0.01 * It)
    dv5 = data_vectors(d5)
    algo = new_algo(numContribs=40, numReps=1, maxIterations=250, convergenceCriterion=1e-9)
    algo.model = me; algo.data = d5
    spec5 = dict(model="ellcs", n_contrib=40, lo=[1e-9, 2e-9, 2e-10], hi=[5e-8, 1e-7, 1e-8], gen=[1, 1, 1],
                 comp_exp=0.6666666, max_iter=250, conv_crit=1e-9, eta_c=me.eta_c(), eta_s=me.eta_s(),
                 eta_sol=me.eta_sol(), int_div=100)
    save_traj("g4_ellcs_q40.npz", dv5, spec5, run_mcfit(algo, 40, 1005))

    # T7..T10: the four plugin models outside the BASELINE configs, short runs
    q_nm = np.logspace(np.log10(0.02), np.log10(2.0), 40)
    dtmp = sasdata(q_nm, np.ones(40), 0.01 * np.ones(40))

    def short_traj(tag, model, names, lo, hi, gen, truth, fname, extra_spec):
        for n, l, h in zip(names, lo, hi):
            getattr(model, n).setActive(True)
            getattr(model, n).setActiveRange((l, h))
        It = np.array(model.calc(dtmp, truth, 0.6666666).cumInt)
        It = It / It.max() * 1e3
        dd = sasdata(q_nm, It * (1 + 0.01 * rs.normal(size=40)), 0.01 * It)
        algo = new_algo(numContribs=40, numReps=1, maxIterations=250, convergenceCriterion=1e-9)
        algo.model = model; algo.data = dd
        spec = dict(model=tag, n_contrib=40, lo=lo, hi=hi, gen=gen, comp_exp=0.6666666, max_iter=250, conv_crit=1e-9)
        spec.update(extra_spec)
        save_traj(fname, data_vectors(dd), spec, run_mcfit(algo, 40, 1100 + len(fname)))

    mei = EllipsoidsIsotropic()
    short_traj("elliso", mei, ["a", "aspect"], [1e-9, 0.2], [5e-8, 20.0], [1, 1],
               np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(0.5, 5, 30)], axis=1), "g4_elliso_q40.npz",
               dict(sld=mei.sld(), int_div=100))
    msc = SphericalCoreShell()
    short_traj("sphcs", msc, ["radius", "t"], [1e-9, 2e-10], [5e-8, 1e-8], [1, 1],
               np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(5e-10, 5e-9, 30)], axis=1), "g4_sphcs_q40.npz",
               dict(eta_c=msc.eta_c(), eta_s=msc.eta_s(), eta_sol=msc.eta_sol()))
    mgc = GaussianChain()
    short_traj("gausschain", mgc, ["rg", "bp"], [1e-9, 1e-9], [1e-7, 1e-6], [1, 0],
               np.stack([rs.uniform(3e-9, 4e-8, 30), rs.uniform(1e-8, 5e-7, 30)], axis=1), "g4_gausschain_q40.npz",
               dict(etas=mgc.etas(), k=mgc.k()))
    mlm = LMADenseSphere()
    short_traj("lmasphere", mlm, ["radius", "volFrac"], [1e-9, 0.01], [5e-8, 0.4], [0, 0],
               np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(0.05, 0.3, 30)], axis=1), "g4_lmasphere_q40.npz",
               dict(sld=mlm.sld(), mf=mlm.mf()))

    # T6: Kholodenko worm (3 active), tiny (QUADPACK is slow)
    q_nm = np.logspace(np.log10(0.02), np.log10(2.0), 24)
    mk = Kholodenko()
    dtmp = sasdata(q_nm, np.ones(24), 0.01 * np.ones(24))
    truth = np.stack([rs.uniform(1e-9, 3e-9, 8), rs.uniform(1e-8, 4e-8, 8), rs.uniform(2e-7, 8e-7, 8)], axis=1)
    It = np.array(mk.calc(dtmp, truth, 0.6666666).cumInt)
    It = It / It.max() * 1e3
    d6 = sasdata(q_nm, It * (1 + 0.01 * rs.normal(size=24)), 0.01 * It)
    dv6 = data_vectors(d6)
    algo = new_algo(numContribs=16, numReps=1, maxIterations=40, convergenceCriterion=1e-9)
    algo.model = mk; algo.data = d6
    spec6 = dict(model="kholodenko", n_contrib=16,
                 lo=[min(p.activeRange()) for p in mk.activeParams()],
                 hi=[max(p.activeRange()) for p in mk.activeParams()], gen=[1, 0, 0],
                 comp_exp=0.6666666, max_iter=40, conv_crit=1e-9)
    save_traj("g4_kho_q24.npz", dv6, spec6, run_mcfit(algo, 16, 1006))


def gen_analyse():
    """Whole analyse(): several reps drawing from ONE global stream, incl. retries
    (mcsas.py:214-246) and the result dict (mcsas.py:268-285) + histogram (G5)."""
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    dv = data_vectors(d)
    out = {"data_" + k: v for k, v in dv.items()}
    # A: 3 reps converging at crit=5 (fast), histogram with 2 ranges
    m = Sphere(); m.radius.setActiveRange(tuple(d.sphericalSizeEst()))
    lo, hi = m.radius.activeRange()
    m.radius.histograms().append(Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
    m.radius.histograms().append(Histogram(m.radius, lo, hi, binCount=12, xscale='lin', yweight='num'))
    algo = new_algo(numContribs=150, numReps=3, maxIterations=100000, convergenceCriterion=5.0)
    algo.model = m; algo.data = d
    quiet_logging(None)
    np.random.seed(2001)
    algo.calc()
    res = algo.result[0]
    out["A_lo"] = lo; out["A_hi"] = hi
    out["A_contribs"] = np.array(res["contribs"])
    out["A_fitMean"] = np.array(res["fitMeasValMean"]); out["A_fitStd"] = np.array(res["fitMeasValStd"])
    out["A_scaling"] = np.array(res["scaling"]); out["A_background"] = np.array(res["background"])
    out["A_numIter"] = float(res["numIter"])
    total = int(np.sum(150 + 0))  # placeholder, real consumption below
    # consumed draws: per rep 150 + numIter_r ; we only know the mean -> recover from stream state
    st = np.random.get_state()
    # find consumed count by matching the next draw against a long replay of the same seed
    nxt = np.random.random_sample()
    long = np.random.RandomState(2001).random_sample(2_000_000)
    pos = int(np.nonzero(long == nxt)[0][0])
    out["A_consumed"] = pos
    out["A_stream"] = long[:pos + 8]
    for hi_, h in enumerate(m.radius.histograms()):
        out["A_h%d_edges" % hi_] = np.array(h.xLowerEdge)
        out["A_h%d_bins_full" % hi_] = np.array(h.bins.full)
        out["A_h%d_bins_mean" % hi_] = np.array(h.bins.mean)
        out["A_h%d_bins_std" % hi_] = np.array(h.bins.std)
        out["A_h%d_cdf_mean" % hi_] = np.array(h.cdf.mean)
        out["A_h%d_cdf_std" % hi_] = np.array(h.cdf.std)
        out["A_h%d_obs" % hi_] = np.array(h.observability)
        out["A_h%d_moments" % hi_] = np.array(h.moments.fields, dtype=float)
    out["A_h_spec"] = np.array([[20, 1, 0], [12, 0, 1]])  # binCount, xscale(log=1), yweight idx(vol,num,int,surf)

    # B: retries: maxIterations=60, maxRetries=2, showIncomplete -> 3 attempts per rep, 2 reps
    m2 = Sphere(); m2.radius.setActiveRange(tuple(d.sphericalSizeEst()))
    algo = new_algo(numContribs=50, numReps=2, maxIterations=60, convergenceCriterion=1e-9,
                    maxRetries=2, showIncomplete=True)
    algo.model = m2; algo.data = d
    np.random.seed(2002)
    algo.result = []; algo.stop = False
    algo.analyse()
    res = algo.result[0]
    nxt = np.random.random_sample()
    long = np.random.RandomState(2002).random_sample(100000)
    pos = int(np.nonzero(long == nxt)[0][0])
    out["B_consumed"] = pos
    out["B_stream"] = long[:pos + 8]
    out["B_contribs"] = np.array(res["contribs"])
    out["B_fitMean"] = np.array(res["fitMeasValMean"]); out["B_fitStd"] = np.array(res["fitMeasValStd"])
    out["B_scaling"] = np.array(res["scaling"]); out["B_background"] = np.array(res["background"])
    out["B_numIter"] = float(res["numIter"])
    np.savez_compressed(os.path.join(OUT, "g45_analyse.npz"), **out)
    print("G4/G5 analyse written: A consumed", out["A_consumed"], "numIter", out["A_numIter"],
          "B consumed", out["B_consumed"])


# ---------------------------------------------------------------- G7 (beam-profile smearing)
class _LogspaceCompat(object):
    """SmearingConfig.setIntPoints passes `num = numpy.ceil(n / 2.)` (a float) to numpy.logspace
    (dataobj/sasconfig.py:133, :220).  numpy < 1.18 truncated it to int; numpy 2 raises TypeError, for
    slit as well as pinhole collimation because that line runs first in both.  This context manager
    gives numpy.logspace the old behaviour while the reference's smearing code runs, nothing else."""
    def __enter__(self):
        self._orig = np.logspace
        def logspace(start, stop, num=50, *a, **kw):
            return self._orig(start, stop, int(num), *a, **kw)
        np.logspace = logspace
        return self

    def __exit__(self, *exc):
        np.logspace = self._orig


def gen_smearing():
    from mcsas.dataobj.sasconfig import GaussianSmearing
    out = {}
    cases = (("trapz_slit", "trapezoid", False, dict(umbra=2e7, penumbra=4e7)),
             ("trapz_pinhole", "trapezoid", True, dict(umbra=1.5e7, penumbra=5e7)),
             ("gauss_slit", "gaussian", False, dict(variance=1.2e7)))
    radii = (2e-9, 2.17e-8, 9e-8)
    lma = ((1.5e-8, 0.1), (4e-8, 0.3))
    pset = np.random.RandomState(7).uniform(3e-9, 9e-8, 12).reshape(12, 1)
    with _LogspaceCompat():
        for tag, kind, two_d, prm in cases:
            d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
            if kind == "gaussian":
                d.config.smearing = GaussianSmearing()
                d.config.smearing.updateSmearingLimits(d.x0.binnedData)
            sm = d.config.smearing
            sm.doSmear.setValue(True); sm.twoDColl.setValue(two_d)
            if kind == "trapezoid":
                # penumbra's range follows umbra (sasconfig.py:178-182): set the larger one first
                sm.penumbra.setValue(prm["penumbra"]); sm.umbra.setValue(prm["umbra"])
                sm.penumbra.setValue(prm["penumbra"])
                assert sm.umbra() == prm["umbra"] and sm.penumbra() == prm["penumbra"], (sm.umbra(), sm.penumbra())
            else:
                sm.variance.setValue(prm["variance"])
                assert sm.variance() == prm["variance"]
            assert sm.inputValid()
            d.locs = d.config.prepareSmearing(d.x0.binnedData)       # sasdata.py:165
            dv = data_vectors(d)
            qoff, wts = sm.prepared
            pre = tag + "_"
            out[pre + "q"] = dv["q"]; out[pre + "q_offset"] = np.array(qoff, float)
            out[pre + "weights"] = np.array(wts, float); out[pre + "locs"] = np.array(d.locs, float)
            out[pre + "n_steps"] = int(sm.nSteps())
            for k, v in prm.items():
                out[pre + k] = float(v)
            m = Sphere()
            rows = []
            for r in radii:
                m.radius.setValue(r)
                it, v, w, s = m.calcIntensity(d, compensationExponent=0.6666666)
                rows.append(np.array(it, float))
            out[pre + "sphere_radii"] = np.array(radii); out[pre + "sphere_it"] = np.array(rows)
            m.radius.setActive(True)
            md = m.calc(d, pset, 0.6666666)
            out[pre + "sphere_pset"] = pset; out[pre + "sphere_cum"] = np.array(md.cumInt, float)
            ml = LMADenseSphere()
            rows = []
            for r, vf in lma:
                ml.radius.setValue(r); ml.volFrac.setValue(vf)
                it, v, w, s = ml.calcIntensity(d, compensationExponent=0.6666666)
                rows.append(np.array(it, float))
            out[pre + "lma_params"] = np.array(lma); out[pre + "lma_it"] = np.array(rows)
            out[pre + "lma_fixed"] = np.array([ml.mf(), ml.sld()])
            # a model that cannot smear ignores the configuration (sasmodel.py:57)
            mg = GaussianChain()
            it, v, w, s = mg.calcIntensity(d, compensationExponent=0.6666666)
            out[pre + "gauss_chain_it"] = np.array(it, float)
            if tag == "trapz_slit":
                # one Monte-Carlo chain on smeared intensities (mcFit with data.locs in force)
                ms = Sphere(); ms.radius.setActiveRange(tuple(d.sphericalSizeEst()))
                algo = new_algo(numContribs=60, numReps=1, maxIterations=500, convergenceCriterion=1e-9)
                algo.model = ms; algo.data = d
                spec = dict(model="sphere", n_contrib=60, lo=[min(ms.radius.activeRange())],
                            hi=[max(ms.radius.activeRange())], gen=[0], comp_exp=0.6666666, max_iter=500,
                            conv_crit=1e-9, sld=ms.sld())
                save_traj("g7_sphere_q100_smeared.npz", dv, spec, run_mcfit(algo, 60, 1201),
                          extra=dict(smear_kind="trapezoid", smear_two_d=0, smear_n_steps=int(sm.nSteps()),
                                     smear_umbra=prm["umbra"], smear_penumbra=prm["penumbra"]))
    np.savez_compressed(os.path.join(OUT, "g7_smearing.npz"), **out)
    print("g7_smearing.npz", sorted(out)[:6], "...")


# ---------------------------------------------------------------- G8 (input preparation)
def gen_input_prep():
    out = {}
    rs = np.random.RandomState(11)
    # (a) the reference's demo file, default 100 bins; (b) a dense synthetic curve, 60 bins, with
    # bins of 1, 2 and many points, a missing uncertainty column and a non-finite uncertainty
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    q_nm = np.sort(np.concatenate([np.logspace(-2, 0.4, 1400), np.linspace(0.0101, 0.0109, 3)]))
    I = 1e3 * q_nm ** -3.2 * (1 + 0.05 * rs.standard_normal(len(q_nm))) + 2.0
    sig = 0.02 * I * rs.uniform(0.2, 3.0, len(q_nm))
    sig[17] = np.inf
    d2 = SASData(title="dense", rawArray=np.stack([q_nm, I, sig], axis=1))
    for tag, dd, nb in (("demo", d, 100), ("dense", d2, 60)):
        dd.config.nBin.setValue(nb)
        dd._prepareUncertainty()                      # what the fuMin callback runs (dataobj.py:175, dataconfig.py:117)
        dd._propagateMask()
        dd._reBin()
        out[tag + "_nbin"] = nb
        out[tag + "_fu_min"] = float(dd.config.fuMin())
        out[tag + "_raw_f"] = np.array(dd.f.siData, float)
        out[tag + "_raw_fu"] = np.array(dd.f.unit.toSi(dd.f.rawDataU), float)
        out[tag + "_si_fu"] = np.array(dd.f.siDataU, float)
        out[tag + "_san_x"] = np.array(dd.x0.sanitized, float)
        out[tag + "_san_f"] = np.array(dd.f.sanitized, float)
        out[tag + "_san_fu"] = np.array(dd.f.sanitizedU, float)
        out[tag + "_bin_x"] = np.array(dd.x0.binnedData, float)
        out[tag + "_bin_f"] = np.array(dd.f.binnedData, float)
        out[tag + "_bin_fu"] = np.array(dd.f.binnedDataU, float)
        print("g8", tag, "sanitized", len(dd.x0.sanitized), "->", len(dd.x0.binnedData), "bins")
    np.savez_compressed(os.path.join(OUT, "g8_input_prep.npz"), **out)


# ---------------------------------------------------------------- G9 (round 2: full-size replays)
def model_truth_data(model, q_nm, truth, rs, noise=0.01):
    """Synthetic curve from the REFERENCE's own model.calc on a known population, 1 % uncertainty."""
    n = len(q_nm)
    dtmp = sasdata(q_nm, np.ones(n), 0.01 * np.ones(n))
    It = np.array(model.calc(dtmp, truth, 0.6666666).cumInt)
    It = It / It.max() * 1e3
    return sasdata(q_nm, It * (1 + noise * rs.normal(size=n)), noise * It)


def kholodenko_file_data(nbin):
    """What the reference's loader + input preparation give for testdata/sasfit_kho-1-10-1000.dat
    (datafile/__init__.py:29-46, dataobj/dataobj.py:204-227,288-345): the file's uncertainty column is
    -1, so the 1 % floor (fuMin) is what survives _prepareUncertainty; nbin = 0 keeps the 501 rows."""
    d = loaddatafile("/root/reference/testdata/sasfit_kho-1-10-1000.dat").getDataObj()
    d.config.nBin.setValue(nbin)
    d._prepareUncertainty()
    d._propagateMask()
    d._reBin()
    return d


def gen_big_trajectories():
    """Replays at the BASELINE.json shapes of configs 3 and 4 (and a mid-size Kholodenko chain on the
    reference's own worm data file), so that the window / group / row-table paths of the GPU kernels
    are pinned by the reference itself and not only against each other."""
    rs = np.random.RandomState(2025)
    # config 3 shape: isotropic cylinders, radius + aspect active, 512 q x 400 contributions, 2000 steps
    q_nm = np.logspace(np.log10(0.01), np.log10(3.0), 512)
    mc = CylindersIsotropic(); fix_intdiv(mc)
    mc.radius.setActive(True); mc.aspect.setActive(True)
    mc.radius.setActiveRange((1e-9, 1e-7)); mc.aspect.setActiveRange((0.5, 20.0))
    truth = np.stack([rs.uniform(3e-9, 4e-8, 40), rs.uniform(1, 8, 40)], axis=1)
    d = model_truth_data(mc, q_nm, truth, rs)
    algo = new_algo(numContribs=400, numReps=1, maxIterations=2000, convergenceCriterion=1e-9)
    algo.model = mc; algo.data = d
    spec = dict(model="cyl_aspect", n_contrib=400, lo=[1e-9, 0.5], hi=[1e-7, 20.0], gen=[1, 1],
                comp_exp=0.6666666, max_iter=2000, conv_crit=1e-9, sld=mc.sld(), int_div=100)
    save_traj("g9_cyl_q512.npz", data_vectors(d), spec, run_mcfit(algo, 400, 3003))

    # config 4 shape: core-shell ellipsoid, a / b / t active, 1024 q x 1000 contributions, 1500 steps
    q_nm = np.logspace(np.log10(0.01), np.log10(3.0), 1024)
    me = EllipsoidalCoreShell()
    me.a.setActive(True); me.b.setActive(True); me.t.setActive(True)
    me.a.setActiveRange((1e-9, 1e-7)); me.b.setActiveRange((2e-9, 2e-7)); me.t.setActiveRange((2e-10, 1e-8))
    truth = np.stack([rs.uniform(3e-9, 3e-8, 40), rs.uniform(5e-9, 6e-8, 40), rs.uniform(5e-10, 5e-9, 40)], axis=1)
    d = model_truth_data(me, q_nm, truth, rs)
    algo = new_algo(numContribs=1000, numReps=1, maxIterations=1500, convergenceCriterion=1e-9)
    algo.model = me; algo.data = d
    spec = dict(model="ellcs", n_contrib=1000, lo=[1e-9, 2e-9, 2e-10], hi=[1e-7, 2e-7, 1e-8], gen=[1, 1, 1],
                comp_exp=0.6666666, max_iter=1500, conv_crit=1e-9, eta_c=me.eta_c(), eta_s=me.eta_s(),
                eta_sol=me.eta_sol(), int_div=100)
    save_traj("g9_ellcs_q1024.npz", data_vectors(d), spec, run_mcfit(algo, 1000, 3004))

    # Kholodenko on the reference's worm data, default 1 % floor, 64 log bins (some stay empty), 64
    # contributions, 300 steps, the model's default active ranges (kholodenko.py:57-71)
    d = kholodenko_file_data(64)
    mk = Kholodenko()
    n = 64
    algo = new_algo(numContribs=n, numReps=1, maxIterations=300, convergenceCriterion=1e-9)
    algo.model = mk; algo.data = d
    spec = dict(model="kholodenko", n_contrib=n,
                lo=[min(p.activeRange()) for p in mk.activeParams()],
                hi=[max(p.activeRange()) for p in mk.activeParams()], gen=[1, 0, 0],
                comp_exp=0.6666666, max_iter=300, conv_crit=1e-9)
    save_traj("g9_kho_q64.npz", data_vectors(d), spec, run_mcfit(algo, n, 3006))


def gen_kholodenko_config5(steps=300, fname="g9_kho_q512.npz"):
    """BASELINE config 5 AS NAMED: the Kholodenko fit on testdata/sasfit_kho-1-10-1000.dat at 512 q x
    600 contributions.  The file has 501 rows; the 512-point grid is the loader's (q, I) interpolated
    log-log onto logspace(q_min, q_max, 512) with sigma = 1 % I.  QUADPACK makes this slow
    (~0.8 ms per q per form factor: ~4 min for the initial set, ~0.8 s per step).  Round 5: `kho5_long` stores the same
    chain (same seed, same stream: its first 300 steps ARE g9_kho_q512) over 1300 steps = more than two sweeps over the 600
    contributions, so that every contribution is proposed again after it may have been replaced (g9_kho_q512_long.npz)."""
    d0 = kholodenko_file_data(0)
    q0 = np.array(d0.x0.unit.toDisplay(d0.q) if hasattr(d0.x0.unit, "toDisplay") else d0.q * 1e-9, dtype=float)
    I0 = np.array(d0.f.binnedData, dtype=float)
    assert len(q0) == 501 and np.all(np.diff(q0) > 0)
    sig0 = np.array(d0.f.binnedDataU, dtype=float)
    np.testing.assert_allclose(sig0, 0.01 * I0, rtol=1e-12)           # the 1 % floor is what the loader leaves
    q_nm = np.logspace(np.log10(q0[0]), np.log10(q0[-1]), 512)
    q_nm[0], q_nm[-1] = q0[0], q0[-1]
    I = np.exp(np.interp(np.log(q_nm), np.log(q0), np.log(I0)))
    d = sasdata(q_nm, I, 0.01 * I)
    assert d.count == 512
    mk = Kholodenko()
    n = 600
    algo = new_algo(numContribs=n, numReps=1, maxIterations=steps, convergenceCriterion=1e-9)
    algo.model = mk; algo.data = d
    spec = dict(model="kholodenko", n_contrib=n,
                lo=[min(p.activeRange()) for p in mk.activeParams()],
                hi=[max(p.activeRange()) for p in mk.activeParams()], gen=[1, 0, 0],
                comp_exp=0.6666666, max_iter=steps, conv_crit=1e-9)
    save_traj(fname, data_vectors(d), spec, run_mcfit(algo, n, 3005),
              extra=dict(file_q_nm=q0, file_I=I0))


# ---------------------------------------------------------------- G10 (parameter declarations)
def gen_param_declarations():
    """What the reference's model classes declare (name, default, valueRange, activeRange, generator,
    active flag; utils/parameter.py:577-743, models/*.py) and what McSAS.mcFit's generateParameters sees
    — the mirror classes in mcsas_amd/scatteringmodels and setup_from_model are checked against this."""
    import json
    out = {}
    from mcsas.models.cylindersradiallyisotropic import CylindersRadiallyIsotropic
    classes = (Sphere, CylindersIsotropic, EllipsoidalCoreShell, Kholodenko, EllipsoidsIsotropic,
               SphericalCoreShell, GaussianChain, LMADenseSphere, CylindersRadiallyIsotropic)
    for cls in classes:
        m = cls()
        plist = []
        for p in m.params():
            e = dict(name=p.name(), value=float(p()), fit=bool(hasattr(p, "isActive")))
            vr = p.valueRange() if hasattr(p, "valueRange") else None
            e["valueRange"] = [float(vr[0]), float(vr[1])] if vr is not None else None
            if e["fit"]:
                ar = p.activeRange()
                e["active"] = bool(p.isActive())
                e["activeRange"] = [float(min(ar)), float(max(ar))]
                e["generator"] = p.generator().__name__
            plist.append(e)
        out[cls.__name__] = dict(shortName=cls.shortName, canSmear=bool(getattr(cls, "canSmear", False)),
                                 params=plist, activeParams=[p.name() for p in m.activeParams()])
    with open(os.path.join(OUT, "g10_param_decls.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("G10 written:", ", ".join(out))


# ---------------------------------------------------------------- G14 (round 3): long budgets at the BASELINE config-2 shape
def gen_long_trajectories():
    """512 q x 400 contributions (config 2's shape) replayed over long budgets, so that the kernels' `ft + (new - old)`
    and their lazily re-evaluated rows are held against the reference over 60+ sweeps of the contributions, not 4:
    (a) 25 000 fixed steps; (b) a second data realisation run until the reference itself converges at criterion 2 (a
    chain that ends by convergence, not by budget).  (With positiveBackground the reference's own trajectory hangs on where
    MINPACK stalls next to the |b| kink — it hit maxfev on this very chain — so (b) keeps the default free background.)"""
    q_nm, I, sig = synthetic_sphere_data(512)
    d = sasdata(q_nm, I, sig)
    dv = data_vectors(d)
    m = Sphere(); m.radius.setActiveRange((np.pi / dv["q"].max(), np.pi / dv["q"].min()))
    algo = new_algo(numContribs=400, numReps=1, maxIterations=25000, convergenceCriterion=1e-9)
    algo.model = m; algo.data = d
    spec = dict(model="sphere", n_contrib=400, lo=[min(m.radius.activeRange())], hi=[max(m.radius.activeRange())], gen=[0],
                comp_exp=0.6666666, max_iter=25000, conv_crit=1e-9, sld=m.sld())
    save_traj("g14_sphere_q512_long.npz", dv, spec, run_mcfit(algo, 400, 1401))
    q_nm, I, sig = synthetic_sphere_data(512, seed=77)
    d2 = sasdata(q_nm, I, 2.0 * sig)                          # twice the uncertainty: the chain gets to chi2 <= 2 in ~1e4 steps
    dv2 = data_vectors(d2)
    m2 = Sphere(); m2.radius.setActiveRange((np.pi / dv2["q"].max(), np.pi / dv2["q"].min()))
    algo = new_algo(numContribs=400, numReps=1, maxIterations=100000, convergenceCriterion=2.0)
    algo.model = m2; algo.data = d2
    spec2 = dict(spec); spec2.update(lo=[min(m2.radius.activeRange())], hi=[max(m2.radius.activeRange())], max_iter=100000,
                                     conv_crit=2.0)
    save_traj("g14_sphere_q512_converge.npz", dv2, spec2, run_mcfit(algo, 400, 1402))


# ---------------------------------------------------------------- G13 (round 3): the quick-start fit, free-running
def gen_quickstart(seed=3001):
    """doc/source/quickstart.rst:66-107: Sphere on testdata/quickstartdemo1.csv, radius range from the data
    (sphericalSizeEst), 10 repetitions x 300 contributions, convergence criterion 1, background on, ONE histogram with a
    log x axis (GUI defaults: 50 bins, volume-weighted) — the reference run free (global numpy RNG seeded) through calc(),
    i.e. analyse() + histogram().  Stored: the data vectors, every repetition's parameter set, the histogram's per-bin
    mean / std over the repetitions, CDF, observability, moments, and the wall time of calc() in THIS container (the
    document quotes 36 s on a 2012 iMac, quickstart.rst:106-107)."""
    import time
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    dv = data_vectors(d)
    out = {"data_" + k: v for k, v in dv.items()}
    m = Sphere(); m.radius.setActiveRange(tuple(d.sphericalSizeEst()))
    lo, hi = m.radius.activeRange()
    m.radius.histograms().append(Histogram(m.radius, lo, hi, binCount=50, xscale='log', yweight='vol'))
    algo = new_algo(numContribs=300, numReps=10, maxIterations=100000, convergenceCriterion=1.0)
    algo.model = m; algo.data = d
    quiet_logging(None)
    np.random.seed(seed)
    t0 = time.time()
    algo.calc()
    wall = time.time() - t0
    res = algo.result[0]
    h = m.radius.histograms()[0]
    out.update(lo=lo, hi=hi, seed=seed, wall_s=wall, contribs=np.array(res["contribs"]),
               fitMean=np.array(res["fitMeasValMean"]), fitStd=np.array(res["fitMeasValStd"]),
               scaling=np.array(res["scaling"]), background=np.array(res["background"]), numIter=float(res["numIter"]),
               times=np.array(res["times"]),
               h_edges=np.array(h.xLowerEdge), h_width=np.array(h.xWidth), h_mean=np.array(h.xMean),
               h_bins_full=np.array(h.bins.full), h_bins_mean=np.array(h.bins.mean), h_bins_std=np.array(h.bins.std),
               h_cdf_mean=np.array(h.cdf.mean), h_cdf_std=np.array(h.cdf.std), h_obs=np.array(h.observability),
               h_moments=np.array(h.moments.fields, dtype=float))
    np.savez_compressed(os.path.join(OUT, "g13_quickstart.npz"), **out)
    print("G13 quick start written: calc() %.1f s here, numIter mean %.0f, scaling %s, background %s" %
          (wall, out["numIter"], res["scaling"], res["background"]))


def gen_series(seed=3101):
    """The computational core of the series Calculator (gui/calc.py:271-349): the SAME algorithm and model objects run calc() on
    one data set after the other, and after each one every histogram of every active parameter contributes
    (seriesKeyValue, hist.moments.fields) to the series table under (parameter, range, weighting) (_updateSeries :331-349).
    Two data sets here — the quick-start file and a synthetic tri-modal sphere curve (64 q) — drawn from ONE global stream
    (the second calc() continues where the first stopped), fixed budgets so that every repetition runs its 200 steps.
    Stored: both data sets' vectors, the stream, where each calc() started in it, each result and the series table."""
    d1 = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    d2 = sasdata(*synthetic_sphere_data(64, seed=77, qmin=0.02, qmax=2.0))
    keys = [10.0, 25.0]
    m = Sphere(); m.radius.setActiveRange(tuple(d1.sphericalSizeEst()))
    lo, hi = m.radius.activeRange()
    m.radius.histograms().append(Histogram(m.radius, lo, hi, binCount=16, xscale='log', yweight='vol'))
    m.radius.histograms().append(Histogram(m.radius, lo, 0.5 * hi, binCount=8, xscale='lin', yweight='num'))
    algo = new_algo(numContribs=60, numReps=2, maxIterations=200, convergenceCriterion=1e-9, maxRetries=0, showIncomplete=True)
    algo.model = m
    quiet_logging(None)
    np.random.seed(seed)
    long = np.random.RandomState(seed).random_sample(200000)
    out = dict(lo=lo, hi=hi, keys=np.array(keys), seed=seed)
    series = {}
    starts = [0]
    for i, d in enumerate((d1, d2)):
        for k, v in data_vectors(d).items():
            out["d%d_%s" % (i, k)] = v
        algo.data = d
        algo.calc()
        res = algo.result[0]
        out["d%d_contribs" % i] = np.array(res["contribs"]); out["d%d_numIter" % i] = float(res["numIter"])
        out["d%d_scaling" % i] = np.array(res["scaling"]); out["d%d_background" % i] = np.array(res["background"])
        for h in m.radius.histograms():                      # _updateSeries
            uid = (h.param.name(),) + tuple(h.xrange) + (h.yweight,)
            series.setdefault(uid, []).append((keys[i], np.array(h.moments.fields, dtype=float)))
        st = np.random.get_state()
        nxt = np.random.random_sample()
        np.random.set_state(st)
        starts.append(int(np.nonzero(long == nxt)[0][0]))
    out["starts"] = np.array(starts); out["stream"] = long[:starts[-1] + 8]
    for j, (uid, rows) in enumerate(series.items()):
        out["s%d_uid" % j] = np.array([uid[1], uid[2]]); out["s%d_weight" % j] = uid[3]
        out["s%d_keys" % j] = np.array([r[0] for r in rows]); out["s%d_moments" % j] = np.stack([r[1] for r in rows])
    np.savez_compressed(os.path.join(OUT, "g15_series.npz"), **out)
    print("G15 series written: draws per data set %s, moments %s" % (np.diff(starts), out["s0_moments"][:, 0]))



# ---------------------------------------------------------------- G16 / G17 (round 4)
def _heavy_case(tag, seed_data=7, noise=0.02):
    """(model, data, spec, histogram declarations) of the free-running heavy-model cases: a synthetic curve from the
    REFERENCE's own model.calc on a known population of that model, `noise` relative uncertainty + Gaussian noise."""
    rs = np.random.RandomState(seed_data)
    q_nm = np.logspace(np.log10(0.02), np.log10(2.0), 100)
    if tag == "cyl":
        m = CylindersIsotropic(); fix_intdiv(m)
        m.radius.setActive(True); m.aspect.setActive(True)
        m.radius.setActiveRange((1e-9, 5e-8)); m.aspect.setActiveRange((0.5, 20.0))
        truth = np.stack([rs.uniform(3e-9, 2e-8, 40), rs.uniform(1, 8, 40)], axis=1)
        spec = dict(model="cyl_aspect", lo=[1e-9, 0.5], hi=[5e-8, 20.0], gen=[1, 1], comp_exp=0.6666666, sld=m.sld(), int_div=100)
        hists = [("radius", 1e-9, 5e-8, 16, "log", "vol"), ("aspect", 0.5, 20.0, 10, "log", "vol")]
    elif tag == "ellcs":
        m = EllipsoidalCoreShell()
        m.a.setActive(True); m.b.setActive(True); m.t.setActive(True)
        m.a.setActiveRange((1e-9, 5e-8)); m.b.setActiveRange((2e-9, 1e-7)); m.t.setActiveRange((2e-10, 1e-8))
        truth = np.stack([rs.uniform(3e-9, 2e-8, 40), rs.uniform(5e-9, 4e-8, 40), rs.uniform(5e-10, 5e-9, 40)], axis=1)
        spec = dict(model="ellcs", lo=[1e-9, 2e-9, 2e-10], hi=[5e-8, 1e-7, 1e-8], gen=[1, 1, 1], comp_exp=0.6666666,
                    eta_c=m.eta_c(), eta_s=m.eta_s(), eta_sol=m.eta_sol(), int_div=100)
        hists = [("a", 1e-9, 5e-8, 16, "log", "vol"), ("b", 2e-9, 1e-7, 16, "log", "vol"), ("t", 2e-10, 1e-8, 8, "log", "num")]
    else:
        raise ValueError(tag)
    d = model_truth_data(m, q_nm, truth, rs, noise=noise)
    return m, d, spec, hists, truth


def _free_run(m, d, hists, n_contrib, reps, crit, seed, max_iter=100000):
    """calc() — analyse() + histogram() — of the reference, free-running from the seeded global numpy stream."""
    import time
    for (pname, lo, hi, nb, xs, yw) in hists:
        p = getattr(m, pname)
        p.histograms().append(Histogram(p, lo, hi, binCount=nb, xscale=xs, yweight=yw))
    algo = new_algo(numContribs=n_contrib, numReps=reps, maxIterations=max_iter, convergenceCriterion=crit)
    algo.model = m; algo.data = d
    quiet_logging(None)
    np.random.seed(seed)
    t0 = time.time()
    algo.calc()
    wall = time.time() - t0
    res = algo.result[0]
    out = dict(seed=seed, wall_s=wall, n_contrib=n_contrib, reps=reps, crit=crit, max_iter=max_iter,
               contribs=np.array(res["contribs"]), fitMean=np.array(res["fitMeasValMean"]), fitStd=np.array(res["fitMeasValStd"]),
               scaling=np.array(res["scaling"]), background=np.array(res["background"]), numIter=float(res["numIter"]),
               times=np.array(res["times"]))
    k = 0
    for (pname, lo, hi, nb, xs, yw) in hists:
        h = getattr(m, pname).histograms()[0]
        pre = "h%d_" % k
        out.update({pre + "param": pname, pre + "lo": lo, pre + "hi": hi, pre + "nbin": nb, pre + "xscale": xs, pre + "yweight": yw,
                    pre + "edges": np.array(h.xLowerEdge), pre + "width": np.array(h.xWidth), pre + "xmean": np.array(h.xMean),
                    pre + "bins_full": np.array(h.bins.full), pre + "bins_mean": np.array(h.bins.mean),
                    pre + "bins_std": np.array(h.bins.std), pre + "cdf_mean": np.array(h.cdf.mean),
                    pre + "obs": np.array(h.observability), pre + "moments": np.array(h.moments.fields, dtype=float)})
        k += 1
    out["n_hist"] = k
    return out


def gen_free_running_heavy(which=("cyl", "ellcs", "kho")):
    """G16 — one FREE-RUNNING reference calc() per model with an orientation / contour integral (mcsas.py:191-285 end to end, as
    G13 does for the sphere), at sizes the reference affords here: isotropic cylinders and core-shell ellipsoids 100 q x 200
    contributions x 8 repetitions to criterion 1 on curves of their own model (2 % uncertainty), the worm-like chain 64 log bins
    of testdata/sasfit_kho-1-10-1000.dat x 64 contributions x 3 repetitions to criterion 12 (G16_KHO_CRIT; QUADPACK costs the
    reference 0.43 s per step here and a chain is at chi² 10 after 4000 steps: ~1.5 h for the three).  Stored per case: data vectors,
    model configuration, every repetition's parameter set, fit mean / std, scaling, background, mean iterations, one histogram per
    active parameter (bins per repetition, mean / std, CDF, observability, moments), wall time of calc() here."""
    for tag in which:
        if tag in ("cyl", "ellcs"):
            m, d, spec, hists, truth = _heavy_case(tag)
            out = _free_run(m, d, hists, 200, 8, 1.0, 1601 if tag == "cyl" else 1602)
            out["truth"] = truth
        else:
            # "kho": 64 bins x 64 contributions x 3 repetitions to criterion 12 (round 4); "kho32" (round 5): 32 bins x 48
            # contributions x 12 repetitions to criterion 8 — a pilot with the numpy oracle reaches 9.3 / 6.3 after 1500 steps,
            # 5.0 / 4.5 after 4000 — so that the comparison has twelve reference repetitions behind its standard errors
            big = tag == "kho"
            d = kholodenko_file_data(64 if big else 32)
            m = Kholodenko()
            ap = m.activeParams()
            spec = dict(model="kholodenko", lo=[min(p.activeRange()) for p in ap], hi=[max(p.activeRange()) for p in ap],
                        gen=[1, 0, 0], comp_exp=0.6666666)
            hists = [(p.name(), min(p.activeRange()), max(p.activeRange()), 8, "log" if i == 0 else "lin", "vol") for i, p in enumerate(ap)]
            if big:
                out = _free_run(m, d, hists, 64, 3, float(os.environ.get("G16_KHO_CRIT", "12.0")), 1603, max_iter=20000)
            else:
                out = _free_run(m, d, hists, 48, int(os.environ.get("G16_KHO32_REPS", "12")),
                                float(os.environ.get("G16_KHO32_CRIT", "8.0")), 1604, max_iter=20000)
        out.update({"data_" + k: v for k, v in data_vectors(d).items()})
        out.update({"spec_" + k: np.array(v) for k, v in spec.items()})
        np.savez_compressed(os.path.join(OUT, "g16_%s_free.npz" % tag), **out)
        print("G16 %s: calc() %.1f s here, numIter mean %.0f, scaling %s, background %s" %
              (tag, out["wall_s"], out["numIter"], out["scaling"], out["background"]))


def gen_cyl_radially_isotropic():
    """G18: the one of the reference's three "not verified / unfinished" cylinder variants that runs as written
    (models/cylindersradiallyisotropic.py; cylindersisotropicaspect.py and cylindersradiallyisotropictilted.py raise NameError on
    their first call) — form factor / calc vectors and one short mcFit chain, for the product's run-time plug-in of it."""
    from mcsas.models.cylindersradiallyisotropic import CylindersRadiallyIsotropic
    out = {}
    def fix_div(mm):
        # (the float default breaks numpy.linspace on numpy >= 2, like intDiv: fix_intdiv)
        mm.psiAngleDivisions.setValue(304); mm.psiAngleDivisions.setValue(303)
    m = CylindersRadiallyIsotropic()
    fix_div(m)
    names = ["radius", "psiAngle"]
    psets = [[1e-9, 0.17], [5e-9, 1.3], [2.5e-8, 3.0], [1e-7, 5.9], [3e-10, 0.02]]
    q = np.logspace(7, np.log10(3e9), 48)
    d = sasdata(q * 1e-9, np.ones_like(q), 0.01 * np.ones_like(q))
    qq = np.array(d.q, dtype=float)
    ds = QOnly(qq)
    ff = []
    for pv in psets:
        for n, v in zip(names, pv):
            getattr(m, n).setValue(v)
        ff.append(np.array(m.formfactor(ds), dtype=float))
    cexp = 0.6666666
    md = m.calc(d, np.array(psets, dtype=float), cexp)
    out.update(q=qq, pset=np.array(psets, dtype=float), ff=np.array(ff), cumInt=np.array(md.cumInt), vset=np.array(md.vset),
               wset=np.array(md.wset), sset=np.array(md.sset), comp_exp=cexp,
               rows=np.array([np.array(m.calc(d, np.array([pv], dtype=float), cexp).cumInt) for pv in psets]),
               psi_range=np.array(m.psiAngle.valueRange(), dtype=float), aspect=float(m.aspect()), sld=float(m.sld()),
               divisions=float(m.psiAngleDivisions()))
    np.savez_compressed(os.path.join(OUT, "g18_cylradiso_models.npz"), **out)
    # one short chain, like the other models outside the BASELINE configs (gen_trajectories: short_traj)
    rs = np.random.RandomState(1801)
    q_nm = np.logspace(np.log10(0.02), np.log10(2.0), 40)
    dtmp = sasdata(q_nm, np.ones(40), 0.01 * np.ones(40))
    model = CylindersRadiallyIsotropic()
    fix_div(model)
    lo, hi = [1e-9, 0.05], [5e-8, 6.0]
    for n, l, h in zip(names, lo, hi):
        getattr(model, n).setActive(True)
        getattr(model, n).setActiveRange((l, h))
    truth = np.stack([rs.uniform(3e-9, 2e-8, 30), rs.uniform(0.1, 6.0, 30)], axis=1)
    It = np.array(model.calc(dtmp, truth, cexp).cumInt)
    It = It / It.max() * 1e3
    dd = sasdata(q_nm, It * (1 + 0.01 * rs.normal(size=40)), 0.01 * It)
    algo = new_algo(numContribs=40, numReps=1, maxIterations=250, convergenceCriterion=1e-9)
    algo.model = model; algo.data = dd
    spec = dict(model="cylradiso", n_contrib=40, lo=lo, hi=hi, gen=[1, 0], comp_exp=cexp, max_iter=250, conv_crit=1e-9,
                aspect=model.aspect(), sld=model.sld(), divisions=model.psiAngleDivisions())
    save_traj("g18_cylradiso_q40.npz", data_vectors(dd), spec, run_mcfit(algo, 40, 1802))


def gen_converging_trajectories(which=("cyl", "ellcs", "posbg")):
    """G17 — replayed mcFit chains that END BY CONVERGENCE (mcsas.py:355: `conval > convergenceCriterion` fails) for the cases
    G4 only covers with fixed budgets: a model with an orientation integral (cylinders and core-shell ellipsoids of G16's curves,
    200 contributions, criterion 1) and positiveBackground on the quick-start data (criterion 1)."""
    for tag, seed in (("cyl", 1701), ("ellcs", 1702)):
        if tag not in which:
            continue
        m, d, spec, _, _ = _heavy_case(tag)
        algo = new_algo(numContribs=200, numReps=1, maxIterations=100000, convergenceCriterion=1.0)
        algo.model = m; algo.data = d
        s = dict(spec); s.update(n_contrib=200, max_iter=100000, conv_crit=1.0)
        save_traj("g17_%s_q100_converge.npz" % tag, data_vectors(d), s, run_mcfit(algo, 200, seed))
    if "posbg" not in which:
        return
    # positiveBackground on the quick-start data, whose background is ~0: the fit sits next to the |b| kink all the time and the
    # reference's MINPACK stops up to 1e-6 (relative) above the minimum there (G3 / G4 posbg).  Over thousands of steps that decides
    # a late accept/reject: of nine chains tried (criteria 2 / 1.5 / 1.2 x seeds 1703-1705) the closed-form minimiser of the
    # kernels follows ONE decision for decision to the end (criterion 2, seed 1704: stored as ..._posbg_converge), the call-for-call
    # leastsq restatement all of them.  A second one (criterion 1, seed 1703) is stored as ..._posbg_minpack: the closed form
    # leaves it at accepted move 584 of 606 — the tests replay it with the leastsq restatement and check the kernels up to there.
    d = loaddatafile("/root/reference/testdata/quickstartdemo1.csv").getDataObj()
    for name, crit, seed in (("g17_sphere_q100_posbg_converge.npz", 2.0, 1704), ("g17_sphere_q100_posbg_minpack.npz", 1.0, 1703)):
        m = Sphere(); m.radius.setActiveRange(tuple(d.sphericalSizeEst()))
        algo = new_algo(numContribs=200, numReps=1, maxIterations=100000, convergenceCriterion=crit, positiveBackground=True)
        algo.model = m; algo.data = d
        s = dict(model="sphere", n_contrib=200, lo=[min(m.radius.activeRange())], hi=[max(m.radius.activeRange())], gen=[0],
                 comp_exp=0.6666666, max_iter=100000, conv_crit=crit, sld=m.sld(), find_bg=1, pos_bg=1, from_min=0)
        save_traj(name, data_vectors(d), s, run_mcfit(algo, 200, seed))


def gen_moments_edge_cases():
    """G19 — utils/parameter.py:20-122 (Moments) on weightings the fit never produces but histogram() can: fractions that are all
    zero ('surf' weighting of a model without surface(): variance 0/0 = NaN, and since NaN == 0.0 is False the reference goes on to
    NaN skew / kurtosis), a repetition with no contribution inside the range (skipped: zeros), a one-member range (sigma = 0: skew
    and kurtosis skipped) and an ordinary case."""
    from mcsas.utils.parameter import Moments
    rs = np.random.RandomState(19)
    out = {}
    contribs = rs.uniform(1.0, 10.0, size=(40, 2, 3))
    cases = {"ordinary": (rs.uniform(0.0, 1.0, size=(40, 3)), (2.0, 9.0)),
             "zero_weight": (np.zeros((40, 3)), (2.0, 9.0)),
             "one_rep_zero": (np.concatenate([rs.uniform(0.0, 1.0, size=(40, 2)), np.zeros((40, 1))], axis=1), (2.0, 9.0)),
             "empty_range": (rs.uniform(0.0, 1.0, size=(40, 3)), (20.0, 30.0))}
    c1 = contribs.copy(); c1[:, 0, 1] = 50.0; c1[7, 0, 1] = 5.0            # repetition 1: ONE member inside the range
    with np.errstate(all="ignore"):
        for name, (frac, rng) in cases.items():
            m = Moments(contribs, 0, rng, frac)
            out[name + "_fraction"] = frac; out[name + "_range"] = np.array(rng); out[name + "_fields"] = np.array(m.fields, dtype=float)
        frac = cases["ordinary"][0]
        m = Moments(c1, 0, (2.0, 9.0), frac)
        out["one_member_fraction"] = frac; out["one_member_range"] = np.array((2.0, 9.0)); out["one_member_fields"] = np.array(m.fields, dtype=float)
    out["contribs"] = contribs; out["contribs_one_member"] = c1
    np.savez_compressed(os.path.join(OUT, "g19_moments_edge.npz"), **out)
    for k in sorted(out):
        if k.endswith("_fields"):
            print("G19", k, out[k])


def gen_reference_objects():
    """G20: what the reference's OWN model objects expose once configured through their own setters (the CONFIGS of
    tests/test_model_declarations.py): per parameter what setup_from_model reads (value, isActive, valueRange, activeRange,
    generator), and 64 draws of generateParameters after np.random.seed(5); plus a model of the user's own written against the
    reference's plug-in API (a SASModel with numpy formfactor / volume: the Guinier law of a sphere) and its calc() on 40 q."""
    import json
    sys.path[len(sys.path):] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests")]
    from test_model_declarations import CONFIGS, _configure
    from mcsas.bases.algorithm import numbergenerator as refgen
    classes = {c.__name__: c for c in (Sphere, CylindersIsotropic, EllipsoidalCoreShell, Kholodenko, EllipsoidsIsotropic,
                                       SphericalCoreShell, GaussianChain, LMADenseSphere)}
    gens = {n: getattr(refgen, n) for n in ("RandomUniform", "RandomExponential", "RandomExponential2", "RandomExponential3")}
    flatten = {}
    for cls in sorted(CONFIGS):
        active, fixed, gen_over = CONFIGS[cls]
        m = _configure(classes[cls](), gens, active, fixed, gen_over)
        plist = []
        for p in m.params():
            v = p()
            e = dict(name=p.name(), value=float(v) if isinstance(v, (int, float, np.integer, np.floating)) else None,
                     active=bool(p.isActive()) if callable(getattr(p, "isActive", None)) else None)
            if e["active"]:
                e["valueRange"] = [float(x) for x in p.valueRange()]
                e["activeRange"] = [float(x) for x in p.activeRange()]
                e["generator"] = p.generator().__name__
            plist.append(e)
        np.random.seed(5)
        draws = np.asarray(m.generateParameters(64), dtype=float)
        flatten[cls] = dict(params=plist, draws=draws.tolist())

    from mcsas.bases.algorithm import RandomExponential
    from mcsas.utils.parameter import FitParameter, Parameter
    from mcsas.bases.model import SASModel

    class GuinierSphere(SASModel):
        shortName = "Guinier sphere (user model)"
        parameters = (FitParameter("rg", 5e-9, displayName="radius of gyration", generator=RandomExponential,
                                   valueRange=(1e-10, 1e-6), activeRange=(1e-9, 1e-7)),
                      Parameter("sld", 1e14, displayName="contrast", valueRange=(0., np.inf)))

        def __init__(self):
            super(GuinierSphere, self).__init__()
            self.rg.setActive(True)

        def volume(self):
            r = self.rg() * np.sqrt(5. / 3.)
            return (np.pi * 4. / 3.) * r**3

        def absVolume(self):
            return self.volume() * self.sld()**2

        def formfactor(self, dataset):
            q = self.getQ(dataset)
            return np.exp(-(q * self.rg())**2 / 6.)

    GuinierSphere.factory()
    m = GuinierSphere()
    m.rg.setActiveRange((2e-9, 5e-8))
    q_nm = np.logspace(-2, 0.3, 40)
    d = SASData(title="syn", rawArray=np.stack([q_nm, np.ones(40), 0.01 * np.ones(40)], axis=1))
    d.config.nBin.setValue(0); d._reBin()
    pset = np.array([[3e-9], [1e-8], [4.9e-8], [1e-12], [1.0]])       # the last two are clipped by setValue (valueRange)
    ref = m.calc(d, pset, 0.6666666)
    host = dict(q=np.asarray(m.getQ(d), dtype=float).tolist(), pset=pset.tolist(), comp_exp=0.6666666,
                cumInt=np.asarray(ref.cumInt, dtype=float).tolist(), vset=np.asarray(ref.vset, dtype=float).tolist(),
                wset=np.asarray(ref.wset, dtype=float).tolist())
    with open(os.path.join(OUT, "g20_reference_objects.json"), "w") as f:
        json.dump(dict(flatten=flatten, host_model=host), f, indent=1, sort_keys=True)
    print("G20 written:", ", ".join(flatten))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    quiet_logging(None)
    which = sys.argv[1:] or ["models", "gen", "bgfit", "traj", "analyse", "smear", "prep"]
    if "models" in which:
        gen_model_vectors()
    if "gen" in which:
        gen_generators()
    if "bgfit" in which:
        gen_bgfit()
    if "traj" in which:
        gen_trajectories()
    if "analyse" in which:
        gen_analyse()
    if "smear" in which:
        gen_smearing()
    if "prep" in which:
        gen_input_prep()
    # round 2 additions; "kho5" (~12 min of QUADPACK) only when asked for by name
    if "big" in which or not sys.argv[1:]:
        gen_big_trajectories()
    if "decls" in which or not sys.argv[1:]:
        gen_param_declarations()
    if "kho5" in which:
        gen_kholodenko_config5()
    if "kho5_long" in which:                                   # round 5: two sweeps (~25 min of QUADPACK)
        gen_kholodenko_config5(steps=1300, fname="g9_kho_q512_long.npz")
    if "series" in which:
        gen_series()
    if "quickstart" in which or not sys.argv[1:]:
        gen_quickstart()
    if "long" in which or not sys.argv[1:]:
        gen_long_trajectories()
    # round 4: free-running heavy models (G16; "free_kho" ~ 10-20 min of QUADPACK, only by name) and converging replays (G17)
    if "free" in which or not sys.argv[1:]:
        gen_free_running_heavy(("cyl", "ellcs"))
    if "free_kho" in which:
        gen_free_running_heavy(("kho",))
    if "free_kho32" in which:                                  # round 5: ~30 min of QUADPACK
        gen_free_running_heavy(("kho32",))
    if "converge" in which or not sys.argv[1:]:
        gen_converging_trajectories()
    if "converge_posbg" in which:
        gen_converging_trajectories(("posbg",))
    if "moments" in which or not sys.argv[1:]:
        gen_moments_edge_cases()
    if "cylradiso" in which or not sys.argv[1:]:
        gen_cyl_radially_isotropic()
    if "refobjects" in which or not sys.argv[1:]:
        gen_reference_objects()
