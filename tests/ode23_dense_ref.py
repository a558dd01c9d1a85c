"""CPU reference for ode23 with output at requested times (MATLAB ode23 with
numel(tspan) > 2), the tests' own code: oracle.ode23's loop with the
tspan-vector rules of odearguments / ode23.m and the project's pinned ntrp23.

* t0 = tspan[0], tfinal = tspan[-1], hmax = 0.1*|tfinal - t0|;
* htspan = |tspan[1] - tspan[0]| bounds the initial step only;
* the output times influence nothing else;
* after each accepted step from t to tnew (h = tnew - t) one output per
  pending tspan[next] with tdir*(tnew - tspan[next]) >= 0, in order: ynew
  itself when tspan[next] is tnew bit for bit, else
      c1 = F1*(h*1)
      c2 = ((F1*(h*(-4/3)) + F2*(h*1))      + F3*(h*(4/3)))  + F4*(h*(-1))
      c3 = ((F1*(h*(5/9))  + F2*(h*(-2/3))) + F3*(h*(-8/9))) + F4*(h*1)
      s = (ti - t)/h;  s2 = s*s;  s3 = s2*s
      yi = y + ((c1*s + c2*s2) + c3*s3)
  (ntrp23's BI = [1 -4/3 5/9; 0 1 -2/3; 0 4/3 -8/9; 0 -1 1]).

For a two-point tspan this is oracle.ode23 (test_ode23_dense_cpu.py pins the
accepted times and the final state to it, bit for bit).  `bi` lets a test
plant a wrong interpolation matrix."""
import math
import struct

import numpy as np

from oracle.swrt_oracle import ODE23_A, ODE23_B3, ODE23_E

BI = ((1.0, -4.0 / 3.0, 5.0 / 9.0),
      (0.0, 1.0, -2.0 / 3.0),
      (0.0, 4.0 / 3.0, -8.0 / 9.0),
      (0.0, -1.0, 1.0))


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def ntrp23(ti, t, y, h, f1, f2, f3, f4, bi=BI):
    c1 = f1 * (h * bi[0][0])
    c2 = ((f1 * (h * bi[0][1]) + f2 * (h * bi[1][1])) + f3 * (h * bi[2][1])) + f4 * (h * bi[3][1])
    c3 = ((f1 * (h * bi[0][2]) + f2 * (h * bi[1][2])) + f3 * (h * bi[2][2])) + f4 * (h * bi[3][2])
    s = (ti - t) / h
    s2 = s * s
    s3 = s2 * s
    return y + ((c1 * s + c2 * s2) + c3 * s3)


def ode23_dense(odefun, tspan, y0, rtol=1e-3, atol=1e-6, stats=None, bi=BI, steps_out=None):
    """-> (accepted times, yout, y_final): yout[i] is the solution at tspan[i]
    (row 0 = y0) for len(tspan) > 2, and just [y0, y_final] for two points.
    ``steps_out``: a list that receives (tnew, ynew) of every accepted step."""
    tspan = [float(v) for v in tspan]
    nt = len(tspan)
    t0, tfinal = tspan[0], tspan[-1]
    tdir = math.copysign(1.0, tfinal - t0)
    pow_ = 1.0 / 3.0
    rtol = max(rtol, 100 * np.finfo(float).eps)
    threshold = atol / rtol
    htspan = abs(tspan[1] - tspan[0])
    hmax = 0.1 * abs(tfinal - t0)
    t = t0
    y = np.array(y0, dtype=np.float64)
    f1 = odefun(t, y)
    absh = min(hmax, htspan)
    rh = np.max(np.abs(f1) / np.maximum(np.abs(y), threshold)) / (0.8 * rtol**pow_)
    if absh * rh > 1:
        absh = 1.0 / rh
    absh = max(absh, 16 * np.spacing(t))
    ts = [t]
    yout = [y.copy()]
    nxt = 1
    done = False
    nfailed = 0
    attempts = 0
    while not done:
        hmin = 16 * np.spacing(t)
        absh = min(hmax, max(hmin, absh))
        h = tdir * absh
        if 1.1 * absh >= abs(tfinal - t):
            h = tfinal - t
            absh = abs(h)
            done = True
        nofailed = True
        while True:
            attempts += 1
            y2 = y + f1 * (h * 0.5)
            f2 = odefun(t + h * ODE23_A[0], y2)
            y3 = y + f2 * (h * 0.75)
            f3 = odefun(t + h * ODE23_A[1], y3)
            tnew = t + h * ODE23_A[2]
            if done:
                tnew = tfinal
            h = tnew - t
            ynew = y + (((f1 * (h * ODE23_B3[0])) + f2 * (h * ODE23_B3[1])) + f3 * (h * ODE23_B3[2]))
            f4 = odefun(tnew, ynew)
            fE = ((f1 * ODE23_E[0] + f2 * ODE23_E[1]) + f3 * ODE23_E[2]) + f4 * ODE23_E[3]
            err = absh * np.max(np.abs(fE) / np.maximum(np.maximum(np.abs(y), np.abs(ynew)), threshold))
            if err > rtol:
                nfailed += 1
                if absh <= hmin:
                    raise RuntimeError(f"ode23: step size {absh} below hmin at t={t}")
                if nofailed:
                    nofailed = False
                    absh = max(hmin, absh * max(0.5, 0.8 * (rtol / err) ** pow_))
                else:
                    absh = max(hmin, 0.5 * absh)
                h = tdir * absh
                done = False
            else:
                break
        if nt > 2:
            while nxt < nt and tdir * (tnew - tspan[nxt]) >= 0:
                ti = tspan[nxt]
                yout.append(ynew.copy() if same_bits(ti, tnew) else ntrp23(ti, t, y, h, f1, f2, f3, f4, bi))
                nxt += 1
        if steps_out is not None:
            steps_out.append((tnew, ynew.copy()))
        t = tnew
        y = ynew
        f1 = f4
        ts.append(t)
        if done:
            break
        if nofailed:
            temp = 1.25 * (err / rtol) ** pow_
            if temp > 0.2:
                absh = absh / temp
            else:
                absh = 5.0 * absh
    if nt == 2:
        yout.append(y.copy())
    if stats is not None:
        stats.update(steps=len(ts) - 1, failed=nfailed, attempts=attempts)
    return np.array(ts), np.array(yout), y


def steady_rhs(flow, f, Cg, h, bump):
    """The drivers' odefun (oracle.raytracing_rhs) over ONE gridded flow: what
    the device computes with nslots = 1 (no time blend)."""
    from oracle.swrt_oracle import interpolate

    def odefun(t, y):
        n = y.size // 4
        xx, yy, k1, k2 = y[0:n], y[n:2 * n], y[2 * n:3 * n], y[3 * n:4 * n]
        I = {m: interpolate(xx, yy, flow[m], h, h, bump) for m in ("u", "v", "ux", "uy", "vx", "vy")}
        s = np.sqrt(f**2 + Cg**2 * (k1 * k1 + k2 * k2))
        return np.concatenate([I["u"] + (Cg * k1) / s, I["v"] + (Cg * k2) / s,
                               -(I["ux"] * k1 + I["vx"] * k2), -(I["uy"] * k1 + I["vy"] * k2)])
    return odefun


def low_mode_case(n, seed=7, nx=64):
    """A low-mode streamfunction pair on nx^2 (|U| ~ 0.5) and n packets: smooth
    enough for a tight DOP853 reference, strong enough that ode23 at RelTol
    1e-3 rejects attempts.  Every component of y0 stays away from zero (x in
    [1, 3]^2, k in the first quadrant's middle), so the initial-step heuristic
    max |f| / max(|y|, AbsTol/RelTol) gives a first step of a few 1e-2 and a
    fine output grid can bind it."""
    from oracle import swrt_oracle as orc
    L, f, Cg = 2 * np.pi, 3.0, 1.0
    xs = np.arange(nx) * (L / nx)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    psi1 = 0.15 * (np.cos(2 * X + Y) + np.sin(X - 3 * Y))
    psi2 = 0.15 * (np.cos(2 * X + Y + 0.6) + 1.2 * np.sin(X - 3 * Y - 0.4))
    flows = []
    for psi in (psi1, psi2):
        fl = orc.spectral_scheme_fields(L, nx, psi)
        fl.pop("psi")
        flows.append(fl)
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 3.0, (n, 2))
    th = rng.uniform(np.pi / 8, 3 * np.pi / 8, n)
    kk = rng.uniform(6.0, 12.0, n)
    k = np.stack([kk * np.cos(th), kk * np.sin(th)], axis=1)
    return dict(nx=nx, L=L, f=f, Cg=Cg, flow1=flows[0], flow2=flows[1], psi1=psi1, psi2=psi2, x=x, k=k)


def y_of(x, k):
    return np.concatenate([x[:, 0], x[:, 1], k[:, 0], k[:, 1]])
