"""Group (d) of the mfma_blocks.h tests: one measurement loop over random SPD matrices (condition 1 .. 1e12, unscaled and row-scaled),
run once with the float64 restatements of tests/_mfma_reference.py (on the CPU: the yardstick) and once with the device routines
behind tests/_mfma_probe.py.  Both deliver the same records, so the device's worst figure per (family, size, metric) is compared with
FACTOR times the reference's.

`python -m tests._mfma_accuracy [--device] > profiles/mfma_blocks_reference.txt` writes the table kept under profiles/."""
import functools
import sys

import numpy as np

from tests import _mfma_cases as cases
from tests import _mfma_probe as P
from tests import _mfma_reference as ref

FACTOR = 16.0      # device bound = FACTOR x the reference's worst value per family, size and metric
NCB = 3            # column blocks of the right-hand sides (dealt over the 8 wavefronts of a 512-thread launch)
CHOL16_NCOLS = (16, 12, 6)


class ReferenceBackend:
    name = "float64 restatement"

    def chol16_variants(self, ncols):
        def run(form):
            return lambda blocks: tuple(np.stack(v) for v in zip(*[form(b, ncols) for b in blocks]))
        return [("chol16 register", "chol16 register", run(ref.chol16_register)), ("chol16 panels", "chol16 panels", run(ref.chol16_panels))]

    def blocked_variants(self, nb, n_real):
        def run(mats):
            res = [ref.chol_blocked(m, nb, n_real=n_real) for m in mats]
            return np.stack([r[0] for r in res]), np.stack([np.stack(r[1]) for r in res])
        return [("blocked", "blocked", run)]

    def trsm_variants(self, transpose, nb):
        solve = ref.trsm_bwd if transpose else ref.trsm_fwd
        fam = "trsm_bwd" if transpose else "trsm_fwd"
        return [(fam, fam, lambda L, LI, B: np.stack([solve(l, list(li), nb, b) for l, li, b in zip(L, LI, B)]))]


class DeviceBackend:
    def __init__(self, probe):
        self.probe = probe
        self.name = "device, %s build" % probe.form.decode()
        self.launches = []   # every launch made, for the untouched-cells check

    def _run(self, la):
        self.launches.append(la.run(self.probe))
        return la

    def chol16_variants(self, ncols):
        def run(name, op, **kw):
            def f(blocks):
                la = self._run(cases.chol16_launch(name, op, blocks, **kw))
                return la.get_L(), la.get_X()
            return (name, "chol16 panels" if op == P.CHOL16_MFMA else "chol16 register", f)
        out = [run("chol16_wave(ncols=%d)" % ncols, P.CHOL16, ncols=ncols), run("chol16_wave_mfma(ncols=%d)" % ncols, P.CHOL16_MFMA, ncols=ncols, scratch=True)]
        if ncols in P.CHOL16_N:
            out.append(run("chol16_wave_n<%d>" % ncols, P.CHOL16_N[ncols]))
        return out

    def blocked_variants(self, nb, n_real):
        big = 1 << 20
        ld = 16 * nb + 1
        square = {}

        def sq(name, op, threads):
            def f(mats):
                la = self._run(cases.blocked_launch(name, op, threads, mats, nb, ld, n_real if op == P.CHOL_BLOCKED_WAVE and n_real else big))
                square["L"] = la.get_L()
                return la.get_L(), la.get_LI()
            return (name, "blocked", f)

        def tl(name, op, threads):
            def f(mats):   # the tile layout keeps no diagonal block of L: those come from the square run of the same matrices
                la = self._run(cases.tiles_launch(name, op, threads, mats, nb))
                L = la.get_L()
                for b in range(nb):
                    L[:, 16 * b:16 * b + 16, 16 * b:16 * b + 16] = square["L"][:, 16 * b:16 * b + 16, 16 * b:16 * b + 16]
                return L, la.get_LI()
            return (name, "blocked", f)
        out = []
        if nb <= 3:
            out.append(sq("chol_blocked_wave nb=%d%s" % (nb, " n_real=%d" % n_real if n_real else ""), P.CHOL_BLOCKED_WAVE, 64))
        out.append(sq("chol_blocked nb=%d" % nb, P.CHOL_BLOCKED, 512))
        if nb <= 3:
            out.append(tl("chol_tiles_wave nb=%d" % nb, P.CHOL_TILES_WAVE, 64))
        out.append(tl("chol_tiles nb=%d" % nb, P.CHOL_TILES, 512))
        if n_real and n_real - 16 * (nb - 1) in P.CHOL_TILES_LAST:
            nl = n_real - 16 * (nb - 1)
            out.append(tl("chol_tiles_wave_last<%d> nb=%d" % (nl, nb), P.CHOL_TILES_LAST[nl], 64))
        return out

    def trsm_variants(self, transpose, nb):
        fam = "trsm_bwd" if transpose else "trsm_fwd"
        ops = (P.TRSM_BWD_BLOCKED, P.TRSM_BWD_TILES) if transpose else (P.TRSM_FWD_BLOCKED, P.TRSM_FWD_TILES)

        def run(name, op, ld):
            def f(L, LI, B):
                return self._run(cases.trsm_launch(name, op, 512, L, LI, nb, B, NCB, 16 * (NCB + 1) + 1, ld=ld)).get_X()
            return (name, fam, f)
        return [run("%s_blocked nb=%d" % (fam, nb), ops[0], 16 * nb + 1), run("%s_tiles nb=%d" % (fam, nb), ops[1], None)]


def measure(backend):
    """-> list of records dict(routine, family, size, metric, cls, value, case, where)"""
    rec = []

    def add(routine, family, size, metric, cls, values):
        for case, (v, where) in enumerate(values):
            rec.append(dict(routine=routine, family=family, size=size, metric=metric, cls=int(cls[case]), value=v, case=case, where=where))
    for ncols in CHOL16_NCOLS:
        blocks, cls = cases.spd_batch(1, n_real=ncols if ncols < 16 else None)
        for routine, family, run in backend.chol16_variants(ncols):
            L, X = run(blocks)
            add(routine, family, 16, "factor", cls, [ref.factor_metric(a, l) for a, l in zip(blocks, L)])
            add(routine, family, 16, "inverse", cls, [ref.inverse_metric(x, l) for x, l in zip(X, L)])
    for nb, n_real in cases.BLOCKED_SHAPES:
        mats, cls = cases.spd_batch(nb, n_real=n_real)
        size = n_real or 16 * nb
        first = None
        for routine, family, run in backend.blocked_variants(nb, n_real):
            L, LI = run(mats)
            first = first or (L, LI)
            add(routine, family, size, "factor", cls, [ref.factor_metric(a, l) for a, l in zip(mats, L)])
            add(routine, family, size, "inverse", cls, [max(ref.inverse_metric(li[b], l[16 * b:16 * b + 16, 16 * b:16 * b + 16]) for b in range(nb))
                                                        for l, li in zip(L, LI)])
        L, LI = first   # the solves are judged alone: with the factor and the block inverses this backend returned
        rng = np.random.default_rng(77 + size)
        B = cases.mixed_magnitudes(rng, (len(mats), 16 * nb, 16 * NCB))
        for transpose in (False, True):
            for routine, family, run in backend.trsm_variants(transpose, nb):
                X = run(L, LI, B)
                add(routine, family, size, "solve", cls, [ref.solve_metric(l, x, b, transpose) for l, x, b in zip(L, X, B)])
    return rec


def table(records, key="family"):
    """{(family or routine, size, metric): [worst value per condition class]}"""
    ncls = len(cases.spd_classes())
    out = {}
    for r in records:
        row = out.setdefault((r[key], r["size"], r["metric"]), [0.0] * ncls)
        row[r["cls"]] = max(row[r["cls"]], r["value"])
    return out


@functools.lru_cache(maxsize=None)
def _reference_records():
    return tuple(measure(ReferenceBackend()))


def reference_table():
    return table(_reference_records())


def bounds():
    """{(family, size, metric): FACTOR x the float64 restatement's worst value over all condition classes}"""
    return {k: FACTOR * max(v) for k, v in reference_table().items()}


def format_table(title, tab):
    names = [cases.class_name(*c) for c in cases.spd_classes()]
    lines = [title, "%-34s %-4s %-8s " % ("routine", "n", "metric") + " ".join("%14s" % n for n in names) + "   worst"]
    for (routine, size, metric), row in sorted(tab.items()):
        lines.append("%-34s %-4d %-8s " % (routine, size, metric) + " ".join("%14.2f" % v for v in row) + " %7.2f" % max(row))
    return "\n".join(lines)


def rsqrt_pivots():
    """4096 log-spaced pivots over [1e-280, 1e280] and the exact powers of 4 in that range -> (pivots, exponents k of the 4^k)"""
    ks = np.arange(-465, 466)
    return np.logspace(-280, 280, 4096), ks


def main(argv):
    print("# Componentwise backward errors of the mfma_blocks.h routines in units of u = 2^-53, worst entry over the cases of a condition class")
    print("# (tests/_mfma_accuracy.py; metrics and cases: tests/_mfma_reference.py, tests/_mfma_cases.py).  Device bound in the GPU test: %g x the" % FACTOR)
    print("# reference's worst value of the same family, size and metric.")
    print(format_table("\n== float64 restatements (CPU, correctly rounded sqrt and division) ==", reference_table()))
    if "--device" in argv:
        for build in ("left", "right", "fused"):
            probe = P.load(build)
            print(format_table("\n== device, %s build ==" % probe.form.decode(), table(measure(DeviceBackend(probe)), key="routine")))
            piv, ks = rsqrt_pivots()
            err = ref.rsqrt_relative_error(piv, probe.rsqrt_refined(piv))
            p4 = probe.rsqrt_refined(4.0 ** ks)
            print("rsqrt_refined: worst relative error over %d log-spaced pivots in [1e-280, 1e280]: %.3f u (at %.6e); exact 2^-k on 4^k, k = %d .. %d: %s"
                  % (piv.size, err.max(), piv[int(np.argmax(err))], ks[0], ks[-1], bool(np.array_equal(p4, 2.0 ** -ks))))


if __name__ == "__main__":
    main(sys.argv[1:])
