"""Oracle references for the batched mjData views (tests/test_data.py, tests/test_gpu_data.py).

Inputs: tests/sensor_states.dapg_states -- 4 tasks x 3 env-steps x 4 envs of DAPG grasp states.  For
each case the builder reads what sim.data holds after the env-step (mjstep1 x frame_skip; the arrays
are the last substep's forward's) and after a plain forward of the state: xpos, xquat, site_xpos,
qacc, qfrc_constraint, the counts, and the contact list decoded with efc_force by a numpy
mj_contactForce.  "exact": fp64 inputs; "f32": the inputs rounded to fp32, what aw_set_state /
aw_step hand the GPU -- the GPU tests compare against those, the CPU test asserts that the two agree.
"""
import functools

import numpy as np

import sensor_states as ss

# the tolerance the suite holds constraint quantities to (touch, efc_aref): forces, qfrc_constraint
F_RTOL, F_ATOL = 2e-3, 2e-3
PRESSING = 2e-3            # N: a contact presses when its normal force exceeds this


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-9)


def decode_contacts(o):
    """the oracle's contact list with mj_contactForce's forces (pyramidal cones), as arrays [ncon]"""
    from mj_envs_amd.data import contact_force_np
    c = o.get("contact").reshape(-1, 23)
    ef = o.get("efc_force")
    n = len(c)
    out = dict(dist=c[:, 0].copy(), pos=c[:, 1:4].copy(), normal=c[:, 4:7].copy(), frame=c[:, 4:13].reshape(n, 3, 3).copy(),
               geom1=c[:, 13].astype(int), geom2=c[:, 14].astype(int), dim=c[:, 15].astype(int),
               efc_address=c[:, 16].astype(int), mu=c[:, 18].copy(), force=np.zeros((n, 3)), torsion=np.zeros(n))
    for k in range(n):
        out["force"][k], out["torsion"][k] = contact_force_np(out["dim"][k], out["efc_address"][k], c[k, 18:21], ef)
    return out


def read_data(o):
    sc = o.get("scalars")
    return dict(xpos=o.get("xpos").reshape(-1, 3).copy(), xquat=o.get("xquat").reshape(-1, 4).copy(),
                site_xpos=o.get("site_xpos").reshape(-1, 3).copy(), qacc=o.get("qacc").copy(),
                qfrc_constraint=o.get("qfrc_constraint").copy(),
                counts=np.array([int(sc[0]), int(sc[1]), int(sc[2]), int(sc[3])]), contact=decode_contacts(o))


def oracle_step_data(o, m, P, q, v, w, act, rounded):
    c = ss.ctrl_of(m, act)
    r = ss.f32 if rounded else (lambda a: np.array(a, np.float64))
    q, v, w = r(q).copy(), r(v).copy(), r(w).copy()
    o.mjstep1(r(P), q, v, w, ctrl=r(c), nstep=o.frame_skip)
    return read_data(o)


def oracle_forward_data(o, P, q, v, w):
    o.forward1(ss.f32(P), ss.f32(q), ss.f32(v), ss.f32(w))
    return read_data(o)


@functools.lru_cache(maxsize=None)
def data_refs(env_id):
    """dict: step_exact / step_f32 / fwd_f32 -> [step][env] of read_data() records"""
    d = ss.dapg_states(env_id)
    m, o, P = d["m"], d["o"], d["P"]
    out = dict(step_exact=[], step_f32=[], fwd_f32=[])
    for k in range(len(d["steps"])):
        q, v, w, a = d["qpos"][k], d["qvel"][k], d["warm"][k], d["act"][k]
        for key, rounded in (("step_exact", False), ("step_f32", True)):
            out[key].append([oracle_step_data(o, m, P[e], q[e], v[e], w[e], a[e], rounded) for e in range(ss.N_ENVS)])
        out["fwd_f32"].append([oracle_forward_data(o, P[e], q[e], v[e], w[e]) for e in range(ss.N_ENVS)])
    return out


def contact_keys(g1, g2):
    """(geom1, geom2, index within the pair) per contact, in list order"""
    seen, keys = {}, []
    for a, b in zip(np.asarray(g1).tolist(), np.asarray(g2).tolist()):
        i = seen.get((a, b), 0)
        seen[(a, b)] = i + 1
        keys.append((a, b, i))
    return keys


def force_ok(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)) <= F_ATOL + F_RTOL * np.abs(ref)


def compare_contacts(got, ref, geo_atol=None):
    """match by (geom1, geom2, index within the pair) -> (pressing, misses, same_set, errs):
    pressing: the reference's contacts with normal force > PRESSING; misses: those unmatched or with
    a force component (normal, two tangents, torsion) out of tolerance -- or, with geo_atol =
    (dist, pos, normal), a geometric field out of it -- plus the contacts only `got` has that press;
    errs: |error| of the matched contacts' force components"""
    kg, kr = contact_keys(got["geom1"], got["geom2"]), contact_keys(ref["geom1"], ref["geom2"])
    ig = {k: i for i, k in enumerate(kg)}
    pressing = misses = 0
    errs = []
    for j, k in enumerate(kr):
        press = ref["force"][j, 0] > PRESSING
        pressing += press
        i = ig.get(k)
        if i is None:
            misses += press
            continue
        fg = np.append(got["force"][i], got["torsion"][i])
        fr = np.append(ref["force"][j], ref["torsion"][j])
        ok = force_ok(fg, fr).all() and got["dim"][i] == ref["dim"][j]
        if geo_atol is not None:
            ok = ok and abs(got["dist"][i] - ref["dist"][j]) <= geo_atol[0] and \
                np.abs(got["pos"][i] - ref["pos"][j]).max() <= geo_atol[1] and \
                np.abs(got["normal"][i] - ref["normal"][j]).max() <= geo_atol[2]
        errs.extend(np.abs(fg - fr).tolist())
        misses += press and not ok
    extra = set(kg) - set(kr)
    for k in extra:
        misses += got["force"][ig[k], 0] > PRESSING
    return int(pressing), int(misses), kg == kr, errs
