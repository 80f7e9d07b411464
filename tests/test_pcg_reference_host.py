"""The host reference of the indirect back-end (pcg_reference.py) on its own, no GPU: what entitles it to judge the engine in
test_pcg_reference_gpu.py.

  * cond(M) <= 1e4 in every state a run visits (dense eigenvalues; Gershgorin for `wrap`): the engine's CG solves at the floor
    1e-13 are then exact to ~1e-9 at worst, far below that in practice (next but one point);
  * the exact reference's iterates agree with the CPU oracle (qdldl, same settings, the same events) to 1e-9 -- x, y, pri_res,
    dua_res, the final status, the number of rho updates -- in all four runs;
  * the CG statement of the same iteration stays within 1e-10 of the exact one: ten times under what the GPU is held to;
  * every adaptive-rho decision of R3 lies at least 10 % from its threshold, at least one update happens; the progress monitor
    never fires (a run in which it would raises);
  * the two deliberately wrong statements are seen.  Carried products kept across a rho change (R3): the iterates leave the exact
    ones by more than 1e-6 (measured 0.86 to 220 on the cases with rows; without rows M does not depend on rho and nothing is
    stale).  A preconditioner kept across a rho change: after the DEcrease of rho that ends R4 the CG total of that call is at least
    1.3 times the correct statement's (measured 7.5 / 4.7 / 2.5 on mixed / easy / tiny).  After the INcrease 0.1 -> 2.0 it is
    not: there the stale Jacobi scaling needs half the iterations of the correct one on mixed, 15 % fewer on tiny (M = ... + 2000 a a' over a few equality rows
    is low rank plus a well-conditioned part; scaling by its diagonal spreads the cluster), which is why the GPU test holds
    the CG totals to the statement's from both sides.  Without rows the preconditioner does not depend on rho;
  * `easy` needs at most 6 CG iterations on every step after the third of R1 and R2;
  * every call ends in Max_iter_reached, except on `no-rows`: with m = 0 the relaxed iteration contracts by 0.6 per step
    whatever P is, so 60 steps reach 1e-12 and R1 ends Solved (with check_termination=0 after all 60), as do the last calls of R4
    (alpha = 1: two steps converge).  The oracle agrees; the GPU test asserts the status the reference gives.
  * which structures the linear-solve test may use: cond(M) <= 1e4 through the six events of kkt_events.py."""
import zlib

import numpy as np
import pytest

import kkt_events as ev
import pcg_drive as pd
import pcg_reference as pr

RUNS = ("R1", "R2", "R3", "R4")


def _states(name, run):
    """The reduced matrices a run visits: the host model walked through the run's events / rho updates."""
    calls, _ = pr.cached_run(name, run)
    model = pr.make(name)
    yield "setup", model.M()
    if run == "R3":
        for k, (it, est, hi, lo, update) in enumerate(pr.cached_run(name, run)[1].decisions):
            if update:
                model.update_rho(est)
                yield f"rho update at {it}", model.M()
    if run == "R4":
        for call in calls:
            pr.apply_event(model, call["kind"], call["payload"])
            yield call["event"], model.M()


@pytest.mark.parametrize("name", pr.SMALL)
def test_condition_of_every_state(name):
    worst = 0.0
    for run in RUNS:
        for what, M in _states(name, run):
            c = pr.dense_cond(M)
            worst = max(worst, c)
            assert c <= pr.COND_MAX, (name, run, what, c)
    print(f"{name}: cond(M) <= {worst:.2e}")


def test_condition_of_wrap():
    model = pr.make("wrap")
    c = pr.gershgorin_cond(model.M())
    assert c <= 10.0, c  # (and with it about 20 CG iterations per step)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("name", pr.SMALL)
def test_reference_matches_the_oracle(oracle_lib, name, run):
    calls, model = pr.cached_run(name, run)
    got = pd.drive(oracle_lib, name, run, calls, "qdldl")
    e = pd.errors(got, calls)
    print(f"{name} {run}: {e}")
    assert max(e.values()) <= 1e-9, (name, run, e)
    for g, r in zip(got, calls):
        assert g["status"] == r["status"] and g["iter"] == r["iter"], (name, run, r["event"], g["status"], r["status"], r["margin"])
    if run == "R3":
        assert got[0]["rho_updates"] == calls[0]["rho_updates"] >= 1


@pytest.mark.parametrize("name,run", [(n, r) for n in pr.SMALL for r in RUNS] + [("wrap", "R1")])
def test_cg_statement_stays_near_the_exact_reference(name, run):
    exact, _ = pr.cached_run(name, run)
    cg, mcg = pr.cached_run(name, run, pr.CgAdmm)
    e = pd.errors(cg, exact)
    print(f"{name} {run}: {e}, {mcg.cg_total} CG iterations")
    assert max(e["x"], e["y"]) <= 1e-10, (name, run, e)
    if name != "wrap":  # every iterate, not only those a call ends with
        d = pd.trajectory_distance(cg, exact)
        print(f"    every iterate: {d:.2e}")
        assert d <= 1e-10, (name, run, d)
    assert [c["rho_updates"] for c in cg] == [c["rho_updates"] for c in exact]
    if name == "wrap":
        assert max(mcg.cg_per_step) <= 25
    if name == "easy" and run in ("R1", "R2"):
        assert max(mcg.cg_per_step[3:]) <= 6, mcg.cg_per_step


@pytest.mark.parametrize("name", pr.SMALL)
def test_adaptive_rho_decisions_are_clear(name):
    _, model = pr.cached_run(name, "R3")
    assert len(model.decisions) == 3 and [d[0] for d in model.decisions] == [8, 16, 24]
    assert any(d[4] for d in model.decisions)
    for it, est, hi, lo, update in model.decisions:
        assert abs(est - hi) >= 0.1 * hi and abs(est - lo) >= 0.1 * lo, (name, it, est, hi, lo)
        assert update == (est > hi or est < lo)


def test_the_monitor_is_mirrored():
    """A run shaped so that two evaluations lie 25 apart without the progress asked for raises."""
    model = pr.make("mixed")
    model.solve(30, warm=False)
    with pytest.raises(pr.MonitorFired):
        model.solve(50, check_termination=25)  # near the fixed point of a slow iteration: no halving in 25 steps


def test_statuses():
    for name in pr.SMALL:
        for run in RUNS:
            for call in pr.cached_run(name, run)[0]:
                if name != "no-rows":
                    assert call["status"] == "Max_iter_reached" and min(call["margin"]) > 0 and max(call["margin"]) > 1e3, (name, run, call["event"])
                else:  # a verdict that rounding cannot turn
                    assert max(call["margin"]) > 1e3 or max(call["margin"]) < 0.2, (name, run, call["event"], call["margin"])
    assert pr.cached_run("no-rows", "R1")[0][0]["status"] == "Solved"
    assert pr.cached_run("wrap", "R1")[0][0]["status"] == "Max_iter_reached"


@pytest.mark.parametrize("name", ["mixed", "easy", "tiny"])
def test_stale_carried_products_are_seen(name):
    exact, _ = pr.cached_run(name, "R3")
    bad, _ = pr.reference_run(name, "R3", cls=pr.CgAdmm, trajectory=True, keep_Ax=True)
    assert pd.trajectory_distance(bad, exact) > 1e-6
    assert max(pd.distance(bad[0]["x"], exact[0]["x"]), pd.distance(bad[0]["y"], exact[0]["y"])) > 1e-6  # still there at the end


@pytest.mark.parametrize("name", ["mixed", "easy", "tiny"])
def test_a_stale_preconditioner_is_seen(name):
    good = pr.cached_run(name, "R4", pr.CgAdmm)[1]
    exact, _ = pr.cached_run(name, "R4")
    bad_calls, bad = pr.reference_run(name, "R4", cls=pr.CgAdmm, keep_dinv=True)
    per = lambda model: np.array(model.cg_per_step).reshape(len(pr.R4_EVENTS), pr.R4_ITER).sum(axis=1)
    g, b = per(good), per(bad)
    e = pd.errors(bad_calls, exact)
    assert max(e["x"], e["y"]) <= 1e-9, e  # the iterates do not show it ...
    down, up = pr.R4_EVENTS.index("rho-down"), pr.R4_EVENTS.index("rho")
    print(f"{name}: CG per call {g} / stale {b}")
    assert b[down] >= 1.3 * g[down], (name, g, b)  # ... the count does
    assert np.array_equal(b[:up], g[:up])
    assert b[up] <= g[up] and (name != "mixed" or b[up] < 0.7 * g[up])  # (after the increase: no more, on mixed half)


def test_solve_structures_that_qualify():
    qualified = []
    for name, problem in pr.solve_structures().items():
        conds = []
        w = ev.Workspace(None, problem(), name, zlib.crc32(name.encode()), False,
                         judge=lambda ref, b, out, what: conds.append(pr.dense_cond(pr.reduced_matrix(ref))))
        w.events()
        assert len(conds) == 6 if w.A.shape[0] else 5
        if max(conds) <= pr.COND_MAX:
            qualified.append(name)
    assert tuple(qualified) == pr.SOLVE_QUALIFIED and len(set(qualified) - {"mixed", "tiny"}) >= 1
