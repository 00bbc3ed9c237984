"""k_adj_sweep_tab (csrc/table_sensitivity.h) repeats the backward recursion of k_adj_sweep (csrc/adjoint.h) in a function of its
own, because adjoint.h's kernels keep their instructions.  Nothing else keeps the two in step, so this test does: the text of
the stage loop from its operand loads to the inverse of Huu (the loads, Pvv, Huu with its guard) and the update of pp, pv and
kff must be the same in both, and so must the forward pass's recursion.  A fix to one of them fails here until it is made in
the other."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "lap-time-optimization_amd", "csrc")


def _body(path, name):
    src = open(os.path.join(CSRC, path)).read()
    start = src.index(f"void {name}(")
    end = src.index("\n}\n", start)
    lines = [re.sub(r"\s*//.*", "", ln).strip() for ln in src[start:end].splitlines()]
    return [ln for ln in lines if ln]


def _between(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if ln.startswith(first))
    j = next(k for k, ln in enumerate(lines) if k > i and ln.startswith(last))
    return lines[i:j + 1]


def test_the_two_sweeps_share_their_recursion_line_for_line():
    a, t = _body("adjoint.h", "d_adj_sweep"), _body("table_sensitivity.h", "d_adj_sweep_tab")
    # backward: operand loads .. Huu^-1
    block = ("double Prow[8], Bm[16], Xi[2], Ac[8], Kc[2], Pvv[4];", "const double Hi[4] =")
    assert _between(a, *block) == _between(t, *block) and len(_between(a, *block)) > 30
    # backward: the exchange of pp, gu, gx, kff and the update of pp, pv
    block = ("L.x[g][i] = pp;", "pv[0] = -r2[0] * kf0")
    assert _between(a, *block) == _between(t, *block)
    # forward: e_k, a_{k+1}, nu_{k+1}
    block = ("const double e[2] = {grp_sum(Kc[0] * a + kf[0])", "for (int l = 0; l < 8; l++) nu += Prow[l] * L.x[g][l];")
    assert _between(a, *block) == _between(t, *block) and len(_between(a, *block)) > 8
