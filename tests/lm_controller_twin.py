"""An independent statement of the trust-region controller, fp64 numpy.

Written from SURVEY.md Appendix B.2 (the loop) and B.3 (CGNR), with the constants of the reference's nls_solver.cpp:296-337 (all Ceres 2.1.0 defaults there:
initial radius 1e4, max radius 1e16, min_relative_decrease 1e-3, LM diagonal clamp 1e-6 / 1e32, eta 0.1, 500 CG iterations, function / gradient / parameter tolerance
1e-6 / 1e-10 / 1e-8, stop after the first successful step through the callback of :286-292), plus the two Ceres 2.1.0 rules B.2 leaves out:

  [LMS]  LevenbergMarquardtStrategy::ComputeStep: a radius below min_radius = 1e-32 at the start of an attempt fails the step fatally; TrustRegionMinimizer then ends
         the solve (reported as convergence: "minimum trust region radius reached").
  [HIS]  TrustRegionMinimizer::HandleInvalidStep: ++num_consecutive_invalid_steps; when it reaches max_num_consecutive_invalid_steps = 5 the solve FAILS on that
         step; otherwise the strategy's StepIsInvalid() halves the radius (radius *= 0.5) and leaves the reduction factor alone.  A valid step resets the counter.

Nothing here is taken from the oracle's or the device's controller: the tests hold both against this file.  Every decision returns its MARGIN, the relative
distance of the tested quantity from its threshold, so that a test can require that no decision of a trace was a coin toss.
"""
import numpy as np

MIN_RADIUS, MAX_RADIUS = 1e-32, 1e16                 # [LMS]; B.2 "min(1e16, ...)"
MIN_RELATIVE_DECREASE = 1e-3                         # B.2 "if rho > 1e-3"
PARAMETER_TOLERANCE, FUNCTION_TOLERANCE, GRADIENT_TOLERANCE = 1e-8, 1e-6, 1e-10      # B.2
MIN_DIAG, MAX_DIAG = 1e-6, 1e32                      # B.2 "clamp(|J[:,j]|^2, 1e-6, 1e32)"
ETA, MAX_CG = 0.1, 500                               # B.2 "q_tolerance = eta = 0.1", B.3 "for i = 1..500"
MAX_INVALID = 5                                      # [HIS]

# termination codes of the project's statistics: 0 step limit | 1 convergence | 2 the first-successful-step callback | 3 failure (invalid steps)
# record kinds: 0 the initial tests | 1 a decided attempt | 2 the solve ended at the start of an attempt (radius) | 3 ladder: attempt not decided


def _rel_margin(value, threshold):
    """relative distance of `value` from `threshold` (inf when the threshold is 0 and the value is not)"""
    if threshold == 0.0:
        return np.inf if value != 0.0 else 0.0
    return abs(value - threshold) / abs(threshold)


def _record(kind, st, final, accepted=0, pcg_it=0, cand_cost=0.0, model_change=0.0, rel=0.0, margin=np.inf, what=""):
    return {"kind": kind, "final_": int(final), "accepted": int(accepted), "pcg_it": int(pcg_it), "termination": int(st["termination"]), "cost": st["cost"],
            "cand_cost": cand_cost, "model_change": model_change, "rel": rel, "radius_after": st["radius"], "margin": margin, "what": what}


# ---------------------------------------------------------------- (a) the scalar controller ----------------------------------------------------------------

def init(cost, gradient_entries_above_tolerance, free_parameters, radius0=1e4):
    """B.2 lines 1-3: radius = radius0, nu = 2; stop (CONVERGENCE) when max|g| <= 1e-10, i.e. when no gradient entry exceeds it - or when nothing is free."""
    st = {"cost": float(cost), "radius": float(radius0), "nu": 2.0, "invalid": 0, "successful": 0, "attempts": 0, "done": 0, "termination": 0}
    if free_parameters == 0 or gradient_entries_above_tolerance == 0:        # B.2 "if max|g| <= 1e-10: stop (CONVERGENCE)"
        st["done"] = 1; st["termination"] = 1
    return st, _record(0, st, st["done"], what="init")


def begin(st):
    """[LMS] the radius test at the start of an attempt.  Returns (state, record or None)."""
    st = dict(st)
    if st["radius"] < MIN_RADIUS:                                             # [LMS]
        st["done"] = 1; st["termination"] = 1
        return st, _record(2, st, 1, what="radius")
    return st, None


def decide(st, inp, attempt, lm_steps, stop_first=True):
    """One attempt decided (B.2, the body of the loop after the linear solve).  inp: model_change, step_norm2 = |delta|^2, x_norm2 = |x|^2, cand_cost, cg_it,
    cg_broke (the CG solve stopped on a breakdown: Ceres counts the iteration it broke in), force_invalid, gmax_after (stop_first off: max|g| at the accepted point).
    attempt is 0-based; lm_steps = max_num_iterations."""
    st = dict(st)
    mc = inp["model_change"]
    pcg_it = inp["cg_it"] + (1 if inp.get("cg_broke") else 0)
    final = 0; accepted = 0; rel = 0.0; margin = np.inf; what = ""
    if not np.isfinite(mc) or not (mc > 0.0) or inp.get("force_invalid"):     # B.2 "if <= 0 or non-finite => invalid step"
        st["invalid"] += 1                                                    # [HIS]
        if st["invalid"] >= MAX_INVALID:                                      # [HIS] fails ON the fifth
            st["termination"] = 3; final = 1; what = "invalid-fail"
        else:
            st["radius"] = st["radius"] * 0.5; what = "invalid"               # B.2 "radius *= 0.5"; [HIS] nu untouched
    else:
        st["invalid"] = 0                                                     # [HIS] a valid step resets the counter
        step_norm = np.sqrt(inp["step_norm2"]); x_norm = np.sqrt(inp["x_norm2"])
        thr_p = PARAMETER_TOLERANCE * (x_norm + PARAMETER_TOLERANCE)          # B.2 "if |delta| <= 1e-8 (|x| + 1e-8): stop (CONVERGENCE, x unchanged)"
        cost_change = st["cost"] - inp["cand_cost"]
        thr_f = FUNCTION_TOLERANCE * st["cost"]                               # B.2 "if |cost - cost+| <= 1e-6 cost: stop (CONVERGENCE, x unchanged)"
        if step_norm <= thr_p:
            st["termination"] = 1; final = 1; margin = _rel_margin(step_norm, thr_p); what = "parameter-tolerance"
        elif abs(cost_change) <= thr_f:
            st["termination"] = 1; final = 1; margin = min(_rel_margin(step_norm, thr_p), _rel_margin(abs(cost_change), thr_f)); what = "function-tolerance"
        else:
            rel = cost_change / mc                                            # B.2 "rho = (cost - cost+) / model_change"
            margin = min(_rel_margin(step_norm, thr_p), _rel_margin(abs(cost_change), thr_f), _rel_margin(rel, MIN_RELATIVE_DECREASE))
            if rel > MIN_RELATIVE_DECREASE:                                   # B.2 "if rho > 1e-3"
                accepted = 1; st["cost"] = float(inp["cand_cost"]); st["successful"] += 1
                st["radius"] = min(MAX_RADIUS, st["radius"] / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))      # B.2 radius update of a successful step
                st["nu"] = 2.0                                                # B.2 "nu = 2"
                what = "accept-clip" if 1.0 - (2.0 * rel - 1.0) ** 3 < 1.0 / 3.0 else "accept"
                if stop_first:                                                # B.2 "user callback => SOLVER_TERMINATE_SUCCESSFULLY", nls_solver.cpp:286-292
                    st["termination"] = 2; final = 1
                elif inp.get("gmax_after") is not None and inp["gmax_after"] <= GRADIENT_TOLERANCE:      # B.2's gradient test, at the new point
                    st["termination"] = 1; final = 1; what += "+gradient"
            else:
                st["radius"] = st["radius"] / st["nu"]; st["nu"] = st["nu"] * 2.0; what = "reject"            # B.2 "radius <- radius/nu; nu <- 2 nu"
    if not final and attempt + 1 >= lm_steps:                                 # B.2 "for it = 1..max_num_iterations": the limit, termination stays 0
        final = 1; what += "+limit"
    st["attempts"] += 1; st["done"] = final
    return st, _record(1, st, final, accepted, pcg_it, inp["cand_cost"], mc, rel, margin, what)


def run_script(cost, ngrad, nfree, radius0, lm_steps, attempts, stop_first=True):
    """The serial loop on scripted attempt outcomes: the records in order, the final state, and the radius held at the start of every attempt begun."""
    st, rec = init(cost, ngrad, nfree, radius0)
    records = [rec]; radii = []
    k = 0
    while not st["done"] and k < lm_steps:
        st, rec = begin(st)
        if rec is not None:
            records.append(rec); break
        radii.append(st["radius"])
        st, rec = decide(st, attempts[k], k, lm_steps, stop_first)
        records.append(rec); k += 1
    return records, st, radii


def ladder_radii(radius, nu, B):
    """radius of system j of a batch: what j rejections lead to from (radius, nu), in the arithmetic of B.2's rejection rule"""
    out = []
    for _ in range(B):
        out.append(radius); radius = radius / nu; nu = nu * 2.0
    return out


def run_script_ladder(cost, ngrad, nfree, radius0, lm_steps, attempts, plan, ladder_max=6):
    """The same solve decided in batches (the damping ladder): a batch of B attempts is SET UP for the radii of B-1 rejections in a row and then decided in
    order by decide().  When an attempt is not final and the radius it leaves differs from the one the next system of the batch was set up with, that next attempt is
    NOT decided (record kind 3) and starts a batch of one; when it is equal but below 1e-32, [LMS] ends the solve there (kind 2).  Returns the records in order, the
    final state, the number of kind-3 records, and per batch the list (attempt, system radius) it was set up with (radius None: the batch that found the radius run out)."""
    st, rec = init(cost, ngrad, nfree, radius0)
    records = [rec]; setups = []; resyncs = 0
    k = 0; pi = 0; after_resync = False
    while not st["done"] and k < lm_steps:
        if after_resync:
            B = 1
        else:
            B = plan[min(pi, len(plan) - 1)]; pi += 1
        B = max(1, min(B, ladder_max, lm_steps - k)); after_resync = False
        st, rec = begin(st)
        if rec is not None:
            records.append(rec); setups.append([(k + j, None) for j in range(B)]); break
        lad = ladder_radii(st["radius"], st["nu"], B)
        setups.append([(k + j, lad[j]) for j in range(B)])
        decided = 0
        for j in range(B):
            st, rec = decide(st, attempts[k + j], k + j, lm_steps, True)
            records.append(rec); decided += 1
            if st["done"] or j + 1 >= B:
                break
            if st["radius"] != lad[j + 1]:
                records.append(_record(3, st, 0, what="resync")); resyncs += 1; after_resync = True
                break
            if st["radius"] < MIN_RADIUS:                                      # [LMS], for the attempt that would start now
                st = dict(st); st["done"] = 1; st["termination"] = 1
                records.append(_record(2, st, 1, what="radius")); break
        k += decided
    return records, st, resyncs, setups


# ---------------------------------------------------------------- (c) the damped blocks ----------------------------------------------------------------

def cam_blocks(cdiag, tri, fixed, radius):
    """inv(S H S + clamp(c S^2, 1e-6, 1e32) / radius) of one parameter block in fp64: cdiag = squared column norms c, tri = upper triangle of H row by row,
    S = 1 / (1 + sqrt(c)) (B.2 jacobi_scaling).  A fixed block has no inverse (zeros).  A block that is not positive definite falls back to its diagonal.
    Returns (inverse, condition number of the damped block, fell_back)."""
    cdiag = np.asarray(cdiag, np.float64); n = cdiag.size
    if fixed:
        return np.zeros((n, n)), 1.0, False
    S = 1.0 / (1.0 + np.sqrt(cdiag))                                           # B.2 "scale_j = 1 / (1 + |J[:,j]|)"
    H = np.zeros((n, n)); o = 0
    for i in range(n):
        for j in range(i, n):
            H[i, j] = H[j, i] = tri[o]; o += 1
    M = H * np.outer(S, S)
    M[np.diag_indices(n)] += np.clip(cdiag * S * S, MIN_DIAG, MAX_DIAG) / radius      # B.2 "diag_j = clamp(...); D = sqrt(diag / radius)", B.3 A = J^T J + D^2
    if np.all(np.linalg.eigvalsh(M) > 0.0):
        return np.linalg.inv(M), float(np.linalg.cond(M)), False
    return np.diag(1.0 / np.diag(M)), 1.0, True


def tail_diag(c, S, inv_radius):
    """the LM diagonal of the camera tail as the vector kernels hold it, in float32 operations: D2 = clamp((c S) S, 1e-6, 1e32) * (1 / radius), Minv = 1 / (c S^2 + D2);
    both 0 where S == 0 (a fixed parameter)"""
    f = np.float32
    c = np.asarray(c, f); S = np.asarray(S, f); ir = f(inv_radius)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        cs = (c * S) * S
        d2 = np.minimum(np.maximum(cs, f(1e-6)), f(1e32)) * ir
        minv = f(1.0) / (cs + d2)
    free = S != 0
    return np.where(free, d2, f(0)).astype(f), np.where(free, minv, f(0)).astype(f)


# ---------------------------------------------------------------- (b) the whole loop ----------------------------------------------------------------

def cgnr(Js, r, D2, blocks):
    """B.3: preconditioned CG on A = Js^T Js + D^2, b = Js^T r, x0 = 0, M = the diagonal blocks of A.  Returns (x, iterations counted as Ceres counts them: the
    iteration it stopped or broke in, smallest margin of a stop decision)."""
    n = Js.shape[1]
    b = Js.T @ r
    A_blocks = []; o = 0
    for s in blocks:                                                           # B.3 "M = block-diagonal of A with the parameter-block structure"
        Ab = Js[:, o:o + s].T @ Js[:, o:o + s] + np.diag(D2[o:o + s])
        with np.errstate(all="ignore"):
            A_blocks.append((o, s, np.linalg.inv(Ab) if np.all(np.isfinite(Ab)) else np.full((s, s), np.nan)))
        o += s
    x = np.zeros(n); res = b.copy(); p = np.zeros(n); Q0 = 0.0; rho_prev = 1.0; margin = np.inf      # B.3 "r = b; Q0 = 0"
    i = 0
    with np.errstate(all="ignore"):
        for i in range(1, MAX_CG + 1):                                         # B.3 "for i = 1..500"
            z = np.zeros(n)
            for o, s, Mi in A_blocks:
                z[o:o + s] = Mi @ res[o:o + s]                                 # B.3 "z = M^-1 r"
            rho = res @ z
            if rho == 0.0 or not np.isfinite(rho):                             # Ceres conjugate_gradients_solver.cc: IsZeroOrInfinity(rho) ends the solve (a NaN counted with it)
                break
            p = z.copy() if i == 1 else z + (rho / rho_prev) * p               # B.3 "p = z (i=1) else z + (rho_i / rho_{i-1}) p"
            q = Js.T @ (Js @ p) + D2 * p                                       # B.3 "q = A p"
            pq = p @ q
            if pq <= 0.0 or np.isinf(pq):                                      # B.3 "if pq <= 0 or inf: stop"
                break
            alpha = rho / pq; x = x + alpha * p                                # B.3
            res = (b - (Js.T @ (Js @ x) + D2 * x)) if i % 10 == 0 else res - alpha * q      # B.3 "r = (i % 10 == 0) ? b - A x : r - alpha q"
            Q1 = -(x @ (b + res))                                              # B.3 "Q1 = -x^T (b + r)"
            ratio = i * (Q1 - Q0) / Q1
            margin = min(margin, _rel_margin(ratio, ETA))
            if ratio < ETA:                                                    # B.3 "if i (Q1 - Q0) / Q1 < 0.1: stop"
                break
            Q0 = Q1; rho_prev = rho
    return x, i, margin


def minimize(fun, blocks, x0, max_iterations=50, stop_first=False, radius0=1e4):
    """B.2 on a small dense problem.  fun(x, want_jacobian) -> (residuals, J or None).  Returns a dict: x, trace (one dict per attempt begun: accepted, cg, rho,
    radius_after, what, margin), termination, iterations, successful, initial / final cost, final radius, the smallest margin of the run and the branches reached."""
    x = np.array(x0, np.float64)
    r, J = fun(x, True)
    cost = 0.5 * float(r @ r)                                                  # B.2 "cost = 1/2 |r|^2"
    g = J.T @ r                                                                # B.2 "g = J^T r"
    with np.errstate(all="ignore"):
        gmax = np.max(np.abs(g))
    st, rec = init(cost, 0 if gmax <= GRADIENT_TOLERANCE else 1, x.size, radius0)
    out = {"initial_cost": cost, "trace": [], "branches": [rec["what"]] if st["done"] else [], "margin": np.inf}
    scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))                       # B.2 "scale_j = 1 / (1 + |J[:,j]|) (once)"
    Js = J * scale                                                             # B.2 "J <- J diag(scale)"
    k = 0
    while not st["done"] and k < max_iterations:
        st, rec = begin(st)
        if rec is not None:
            out["branches"].append("radius"); break
        with np.errstate(all="ignore"):
            diag = np.minimum(np.maximum(np.sum(Js * Js, axis=0), MIN_DIAG), MAX_DIAG)      # B.2 "diag_j = clamp(|J[:,j]|^2, 1e-6, 1e32)" (a NaN stays a NaN)
            D = np.sqrt(diag / st["radius"])                                   # B.2 "D = sqrt(diag / radius)"
            y, cg_it, cg_margin = cgnr(Js, r, D * D, blocks)
            step = -y                                                          # B.2 "step = -y"
            Jstep = Js @ step
            mc = -float(Jstep @ (r + 0.5 * Jstep))                             # B.2 "model_change = -(J step)^T (r + 1/2 J step)"
        delta = step * scale; xc = x + delta                                   # B.2 "delta = step . scale; x+ = x + delta"
        inp = {"model_change": mc, "step_norm2": float(delta @ delta), "x_norm2": float(x @ x), "cg_it": cg_it, "cand_cost": 0.0}
        valid = np.isfinite(mc) and mc > 0.0
        if valid:
            rc, _ = fun(xc, False)
            inp["cand_cost"] = 0.5 * float(rc @ rc)                            # B.2 "cost+ = 1/2 |r(x+)|^2"
        probe, prec = decide(st, inp, k, max_iterations, stop_first)
        if prec["accepted"]:                                                   # B.2 "x <- x+; re-evaluate r, J (rescale with the SAME scale), g"
            x = xc; r, J = fun(x, True); Js = J * scale
            with np.errstate(all="ignore"):
                inp["gmax_after"] = np.max(np.abs(J.T @ r))
            probe, prec = decide(st, inp, k, max_iterations, stop_first)
        st = probe
        m = min(prec["margin"], cg_margin) if valid else prec["margin"]
        out["margin"] = min(out["margin"], m)
        out["trace"].append({"accepted": prec["accepted"], "cg": cg_it, "rho": prec["rel"], "radius_after": st["radius"], "what": prec["what"], "margin": m})
        out["branches"].append(prec["what"])
        k += 1
    out.update({"x": x, "termination": st["termination"], "iterations": k, "successful": st["successful"], "final_cost": st["cost"], "final_radius": st["radius"]})
    return out
