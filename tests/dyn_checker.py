"""Dynamics-query checker -- TEST INFRASTRUCTURE ONLY (checker of aw_dynamics / k_dyn).

An fp64 numpy statement of include/adroit_wave.h's definitions, built from the fp64 oracle's forward
(Oracle.forward1) and what it exposes: cdof, subtree_com, cvel, xpos, xipos, site_xpos, qM and the
qfrc_* terms.  Only the derived outputs are computed here:

  mj_jac             column i of a point on body b is zero unless dof i's body is b or an ancestor of
                     b; else jacr = cdof_i[0:3], jacp = cdof_i[3:6] + cdof_i[0:3] x (p - subtree_com[root])
  mj_objectVelocity  (flg_local 0): omega = cvel_b[0:3], v = cvel_b[3:6] + omega x (p - subtree_com[root])
  qMinv              np.linalg.inv(qM)

``dtype``: the precision the derived part is evaluated in, from the oracle's values rounded to it
(float32 gives the rounding floor of an fp32 evaluation of the same formulas).
"""
import numpy as np

PT_BODY, PT_BODYCOM, PT_SITE = 0, 1, 2
OUTPUTS = ("qM", "qMinv", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "xvel", "point_pos", "point_vel", "jacp", "jacr")


def body_dofs(m, b):
    """bool [nv]: the dofs whose body is b or an ancestor of b (a walk of body_parentid)"""
    parent = np.asarray(m.arrays["body_parentid"]).astype(int)
    dof_body = np.asarray(m.arrays["dof_bodyid"]).astype(int)
    chain = set()
    while b > 0:
        chain.add(int(b))
        b = parent[b]
    return np.array([d in chain for d in dof_body.tolist()], bool)


def point_of(m, base, kind, idx):
    """(position, body) of a point record"""
    if kind == PT_SITE:
        return base["site_xpos"][idx], int(np.asarray(m.arrays["site_bodyid"])[idx])
    if kind == PT_BODYCOM:
        return base["xipos"][idx], int(idx)
    if kind == PT_BODY:
        return base["xpos"][idx], int(idx)
    raise ValueError(f"unknown point kind {kind}")


def read_base(o):
    """the oracle's arrays after a forward1, fp64"""
    nv = o.nv
    return dict(cdof=o.get("cdof").reshape(nv, 6).copy(), subtree_com=o.get("subtree_com").reshape(-1, 3).copy(),
                cvel=o.get("cvel").reshape(-1, 6).copy(), xpos=o.get("xpos").reshape(-1, 3).copy(),
                xipos=o.get("xipos").reshape(-1, 3).copy(), site_xpos=o.get("site_xpos").reshape(-1, 3).copy(),
                qM=o.get("qM").reshape(nv, nv).copy(), qfrc_bias=o.get("qfrc_bias").copy(),
                qfrc_passive=o.get("qfrc_passive").copy(), qfrc_actuator=o.get("qfrc_actuator").copy(),
                qfrc_smooth=o.get("qfrc_smooth").copy())


def derive(m, base, points, dtype=np.float64):
    """every aw_dynamics output of one env from read_base()'s arrays, evaluated in ``dtype``"""
    c = lambda a: np.asarray(a).astype(dtype)
    root = np.asarray(m.arrays["body_rootid"]).astype(int)
    cdof, com, cvel = c(base["cdof"]), c(base["subtree_com"]), c(base["cvel"])
    nv, nb, npt = cdof.shape[0], cvel.shape[0], len(points)

    def vel(b, p):
        w = cvel[b, :3]
        return np.concatenate([w, cvel[b, 3:] + np.cross(w, p - com[root[b]])]).astype(dtype)

    out = dict(qM=c(base["qM"]), qfrc_bias=c(base["qfrc_bias"]), qfrc_passive=c(base["qfrc_passive"]),
               qfrc_actuator=c(base["qfrc_actuator"]))
    out["qMinv"] = np.linalg.inv(out["qM"])
    xpos = c(base["xpos"])
    out["xvel"] = np.stack([vel(b, xpos[b]) for b in range(nb)])
    out["point_pos"] = np.zeros((npt, 3), dtype)
    out["point_vel"] = np.zeros((npt, 6), dtype)
    out["jacp"] = np.zeros((npt, 3, nv), dtype)
    out["jacr"] = np.zeros((npt, 3, nv), dtype)
    for k, (kind, idx) in enumerate(points):
        p, b = point_of(m, base, kind, idx)
        p = c(p)
        out["point_pos"][k] = p
        out["point_vel"][k] = vel(b, p)
        on = body_dofs(m, b)
        r = p - com[root[b]]
        for i in np.flatnonzero(on):
            out["jacr"][k, :, i] = cdof[i, :3]
            out["jacp"][k, :, i] = cdof[i, 3:] + np.cross(cdof[i, :3], r)
    return out


def evaluate(o, m, params, qpos, qvel, ctrl, points, dtype=np.float64):
    """the checker's outputs of one env at (params, qpos, qvel) with raw controls ctrl (None: zero)"""
    o.forward1(params, qpos, qvel, np.zeros(o.nv), ctrl)
    return derive(m, read_base(o), points, dtype)


def evaluate_batch(o, m, params, qpos, qvel, ctrl, points, dtype=np.float64):
    """evaluate() per row, stacked: name -> [n, ...]"""
    rows = [evaluate(o, m, params[e], qpos[e], qvel[e], None if ctrl is None else ctrl[e], points, dtype)
            for e in range(len(qpos))]
    return {k: np.stack([r[k] for r in rows]) for k in OUTPUTS}
