// aw_model_host.h -- host side of the model: the flat model table (include/aw_blob.h) -> the device
// tables DModel / MData / SensTab / DataTab (aw_common.h), and the check that the model's dof tree is
// the compiled one of its task (aw_trees.h).
//
// Plain host C++: no HIP runtime call, no kernel, no global state.  Every function returns an AW_*
// code and leaves the message in the caller's string, so this header and a main() are a complete
// program on a machine without a GPU (tests/model_build_check.cc).  Every byte the kernels read
// from the model passes through here; the input is not trusted: an entry that is missing or has
// another length than the dims imply, and a value that is out of range where the host uses it as a
// subscript or a shift count, is AW_EBLOB.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/adroit_wave.h"
#include "../../include/aw_blob.h"
#include "aw_common.h"
#include "aw_trees.h"

namespace aw {

// Reader of one model table.  Array reads take the element count the caller expects; the first read
// that finds its entry missing or of another length is remembered (ok() / error()) and yields
// `count` zeros, so a builder section reads its arrays, then asks once before it uses them.
struct Blob {
  const void* p; size_t n;
  mutable std::string bad = {};   // the first failed read

  bool ok() const { return bad.empty(); }
  const std::string& error() const { return bad; }
  bool has(const char* name) const { aw_blob_entry e; return aw_blob_find(p, n, name, &e); }
  // count < 0: whatever the entry holds (its length is the datum; a missing entry is empty)
  std::vector<double> f(const char* name, long count = -1) const {
    aw_blob_entry e;
    std::vector<double> out;
    const bool found = aw_blob_find(p, n, name, &e);
    const size_t cnt = found ? (size_t)e.rows * (size_t)e.cols : 0;
    if (count >= 0 && (!found || cnt != (size_t)count)) {
      if (bad.empty())
        bad = std::string("model table entry ") + name + (found ? ": " + std::to_string(cnt) + " elements" : std::string(": missing")) +
              ", expected " + std::to_string(count);
      out.resize((size_t)count);
      return out;
    }
    out.resize(cnt);
    const char* d = (const char*)e.data;
    for (size_t i = 0; i < cnt; i++) {
      if (e.kind == 0) { double v; memcpy(&v, d + 8 * i, 8); out[i] = v; }
      else { int32_t v; memcpy(&v, d + 4 * i, 4); out[i] = v; }
    }
    return out;
  }
  std::vector<int> i(const char* name, long count = -1) const {
    std::vector<double> v = f(name, count);
    return std::vector<int>(v.begin(), v.end());
  }
  // object ids: every value in [lo, lim)
  std::vector<int> ids(const char* name, long count, int lim, int lo = 0) const {
    std::vector<int> v = i(name, count);
    for (int x : v)
      if ((x < lo || x >= lim) && bad.empty())
        bad = std::string("model table entry ") + name + ": value " + std::to_string(x) + " out of range";
    return v;
  }
  int dim(const char* name, int dflt = -1) const { return aw_blob_dim(p, n, name, dflt); }
  double opt(const char* name, double dflt) const { return aw_blob_opt(p, n, name, dflt); }
};

template <class T, size_t N, class U>
bool put_arr(T (&dst)[N], const std::vector<U>& v) {
  if (v.size() > N) return false;
  for (size_t i = 0; i < v.size(); i++) dst[i] = (T)v[i];
  return true;
}
#define PUT(name, ...)                                                                        \
  do {                                                                                        \
    if (!put_arr(md.name, __VA_ARGS__)) return fail(AW_EUNSUPPORTED, "model field " #name " exceeds kernel capacity"); \
  } while (0)

inline std::vector<float> tof(const std::vector<double>& v) { return std::vector<float>(v.begin(), v.end()); }

// aw_create's default params of every env: task_param_default, one value per param slot
inline int param_defaults(const Blob& B, int nparam, std::vector<float>& out, std::string& err) {
  const std::vector<double> def = B.f("task_param_default", std::max(nparam, 0));
  if (!B.ok()) { err = B.error(); return AW_EBLOB; }
  out = tof(def);
  return AW_OK;
}

// One build: the outputs, the dims, and what one section leaves for the later ones.  run() calls the
// sections in order; the first nonzero code ends the build.
struct ModelBuild {
  const Blob& B;
  DModel& m; MData& md; SensTab& sens; DataTab& data;
  std::string& err;

  int nq = 0, nv = 0, nu = 0, nbody = 0, njnt = 0, ngeom_all = 0, nsite = 0, ntendon = 0, npair = 0, ncand = 0, nsensor = 0;
  std::vector<int> parent, rootid;              // tree
  std::vector<unsigned long long> bmask;        // dofs moving each body
  std::vector<int> trn;                         // dof of each actuator
  std::vector<int> gtype, gbody;                // every model geom (the render table takes the visual ones too)
  std::vector<double> gpos, gquat, gsize, grb;
  std::vector<int> gmap, ctype, cbody;          // model geom -> collidable geom or -1; the compact list
  std::vector<float> crb;
  std::vector<int> sbody;                       // sites
  std::vector<double> spos, squat;
  std::vector<int> pg1, pg2;                    // unified pair list
  std::vector<float> pmg;
  std::vector<int> stype, sobj, sadr, sitetype; // sensors and the sites' shapes
  std::vector<double> ssize;
  std::vector<int> tidx, pf, po, pc;            // task block
  std::vector<int> rt, rb, rc, rsite;           // render table
  std::vector<double> rp, rq, rs, rr;
  std::vector<float> rcol;

  int fail(int code, const std::string& msg) { err = msg; return code; }
  int reads_ok() { return B.ok() ? AW_OK : fail(AW_EBLOB, B.error()); }

  int run() {
    memset(&m, 0, sizeof(m));
    typedef int (ModelBuild::*Section)();
    for (Section s : {&ModelBuild::dims_and_options, &ModelBuild::tree, &ModelBuild::joints_dofs_actuators,
                      &ModelBuild::geoms_and_sites, &ModelBuild::tendons, &ModelBuild::pair_params,
                      &ModelBuild::pair_classes, &ModelBuild::task_block, &ModelBuild::sensor_table,
                      &ModelBuild::touch_pads, &ModelBuild::render_table, &ModelBuild::colours,
                      &ModelBuild::lights_and_tints, &ModelBuild::overrides_and_draws})
      if (int rc = (this->*s)()) return rc;
    return AW_OK;
  }

  int dims_and_options() {
    nq = B.dim("nq"); nv = B.dim("nv"); nu = B.dim("nu"); nbody = B.dim("nbody"); njnt = B.dim("njnt");
    ngeom_all = B.dim("ngeom"); nsite = B.dim("nsite"); ntendon = B.dim("ntendon");
    npair = B.dim("npair"); ncand = B.dim("ncand"); nsensor = std::max(B.dim("nsensor"), 0);
    if (nq < 0 || nv < 0 || nbody < 0 || B.dim("task_kind") < 0) return fail(AW_EBLOB, "model table lacks dims / task block");
    if (nu < 0 || njnt < 0 || ngeom_all < 0 || nsite < 0 || ntendon < 0 || npair < 0 || ncand < 0)
      return fail(AW_EBLOB, "model table lacks dims / task block");
    // the counts without a kernel capacity: an array of that many elements must fit in the table
    for (int c : {ngeom_all, npair, ncand, nsensor})
      if ((size_t)c > B.n / 4) return fail(AW_EBLOB, "model table dims exceed its size");
    if (nq != nv || njnt != nv) return fail(AW_EUNSUPPORTED, "only hinge/slide joints are supported");
    if (nv > MAXV || nbody > MAXB || nsite > MAXS || ntendon > MAXT || nu > MAXU)
      return fail(AW_EUNSUPPORTED, "model exceeds kernel capacity");
    m.nq = nq; m.nv = nv; m.nu = nu; m.nbody = nbody; m.njnt = njnt; m.nsite = nsite; m.ntendon = ntendon;
    m.timestep = (float)B.opt("timestep", 0.002);
    m.gravity[0] = (float)B.opt("gravity_x", 0); m.gravity[1] = (float)B.opt("gravity_y", 0);
    m.gravity[2] = (float)B.opt("gravity_z", -9.81);
    m.iterations = (int)B.opt("iterations", 100);
    m.tolerance = (float)B.opt("tolerance", 1e-8);
    m.noslip_iterations = (int)B.opt("noslip_iterations", 0);
    m.noslip_tolerance = (float)B.opt("noslip_tolerance", 1e-6);
    m.mpr_tolerance = (float)B.opt("mpr_tolerance", 1e-6);
    m.mpr_iterations = (int)B.opt("mpr_iterations", 50);
    m.mpr_tolerance64 = B.opt("mpr_tolerance", 1e-6);
    m.meaninertia = (float)B.opt("meaninertia", 1);
    // pyramidal cones only: R = max(mjMINVAL, (1 - imp) / imp * diagApprox) per edge row, diagApprox =
    // invweight_tran + friction^2 * invweight_(tran|rot); impratio (the elliptic cones' friction /
    // normal impedance ratio) is restated only at its default 1, where it is the identity
    if (B.opt("impratio", 1) != 1.0) return fail(AW_EUNSUPPORTED, "impratio != 1");
    m.pen_length = (float)B.opt("task_pen_length", 1);
    m.tar_length = (float)B.opt("task_tar_length", 1);
    m.task_kind = B.dim("task_kind"); m.frame_skip = B.dim("task_frame_skip", 1);
    m.horizon = B.dim("task_horizon", 0); m.obs_dim = B.dim("task_obs_dim", 0);
    // the observation is assembled in the row buffer (write_obs): it must fit the fast tier's
    if (m.obs_dim < 0 || m.obs_dim > 64 * FAST_NRL) return fail(AW_EUNSUPPORTED, "observation larger than the row buffer");
    m.success_steps = B.dim("task_success_steps", 25);
    m.nparam = B.dim("task_nparam", 0); m.variation = B.dim("task_variation", 0);
    if (m.nparam < 0) return fail(AW_EBLOB, "negative task_nparam");
    if (m.nparam > MAXP) return fail(AW_EUNSUPPORTED, "too many per-env params");
    m.disableflags = 0;
    m.fault_flrow = -1;
    return AW_OK;
  }

  // bodies: subtree ends (DFS order), levels, dof masks
  int tree() {
    parent = B.i("body_parentid", nbody); rootid = B.i("body_rootid", nbody);
    std::vector<int> dofnum = B.i("body_dofnum", nbody), dofadr = B.i("body_dofadr", nbody);
    std::vector<int> dparent = B.i("dof_parentid", nv);
    std::vector<double> bpos = B.f("body_pos", 3 * nbody), bquat = B.f("body_quat", 4 * nbody);
    std::vector<double> ipos = B.f("body_ipos", 3 * nbody), iquat = B.f("body_iquat", 4 * nbody),
                        mass = B.f("body_mass", nbody), inertia = B.f("body_inertia", 3 * nbody),
                        iw = B.f("body_invweight0", 2 * nbody), stm = B.f("body_subtreemass", nbody);
    if (int rc = reads_ok()) return rc;
    for (int b = 0; b < nbody; b++)
      if (dofnum[b] > MAXJB) return fail(AW_EUNSUPPORTED, "more than MAXJB joints in one body");
    // parents precede their children (the subtree and level loops below, every ancestor walk)
    for (int b = 1; b < nbody; b++)
      if (parent[b] < 0 || parent[b] >= b) return fail(AW_EBLOB, "body_parentid: a body's parent must precede it");
    for (int b = 0; b < nbody; b++)
      if (dofnum[b] > 0 && (dofadr[b] < 0 || dofadr[b] + dofnum[b] > nv)) return fail(AW_EBLOB, "body_dofadr + body_dofnum exceeds nv");
    for (int j = 0; j < nv; j++)
      if (dparent[j] < -1 || dparent[j] >= j) return fail(AW_EBLOB, "dof_parentid: a dof's parent must precede it");
    std::vector<int> send(nbody), depth(nbody, 0);
    for (int b = 0; b < nbody; b++) send[b] = b + 1;
    for (int b = nbody - 1; b > 0; b--) send[parent[b]] = std::max(send[parent[b]], send[b]);
    for (int b = 1; b < nbody; b++) depth[b] = depth[parent[b]] + 1;
    int nlev = 0;
    for (int b = 0; b < nbody; b++) nlev = std::max(nlev, depth[b] + 1);
    if (nlev > MAXLEV) return fail(AW_EUNSUPPORTED, "tree too deep");
    std::vector<int> lstart(nlev + 1, 0), lbody;
    for (int l = 0; l < nlev; l++) {
      lstart[l] = (int)lbody.size();
      for (int b = 0; b < nbody; b++)
        if (depth[b] == l) lbody.push_back(b);
    }
    lstart[nlev] = (int)lbody.size();
    m.nlevel = nlev;
    bmask.assign(nbody, 0);
    std::vector<unsigned long long> amask(nv, 0);
    for (int b = 1; b < nbody; b++) {
      int a = b;
      while (a > 0) {
        for (int k = 0; k < dofnum[a]; k++) bmask[b] |= 1ull << (dofadr[a] + k);
        a = parent[a];
      }
    }
    for (int j = 0; j < nv; j++)
      for (int a = dparent[j]; a >= 0; a = dparent[a]) amask[j] |= 1ull << a;

    PUT(body_parentid, parent); PUT(body_rootid, rootid); PUT(body_dofnum, dofnum);
    PUT(body_dofadr, dofadr); PUT(body_depth, depth); PUT(body_subtree_end, send); PUT(level_start, lstart);
    PUT(level_body, lbody);
    PUT(body_pos, tof(bpos)); PUT(body_quat, tof(bquat));
    PUT(body_ipos, tof(ipos)); PUT(body_iquat, tof(iquat));
    PUT(body_mass, tof(mass)); PUT(body_inertia, tof(inertia));
    PUT(body_invweight0, tof(iw));
    PUT(body_subtreemass, tof(stm));
    PUT(body_dofmask, bmask); PUT(dof_ancmask, amask);
    PUT(body_pos64, bpos); PUT(body_quat64, bquat);
    return AW_OK;
  }

  int joints_dofs_actuators() {
    std::vector<int> jtype = B.i("jnt_type", njnt), jbody = B.i("jnt_bodyid", njnt), jlim = B.i("jnt_limited", njnt);
    std::vector<double> jpos = B.f("jnt_pos", 3 * njnt), jaxis = B.f("jnt_axis", 3 * njnt), jrange = B.f("jnt_range", 2 * njnt),
                        jmargin = B.f("jnt_margin", njnt), jsolref = B.f("jnt_solref", 2 * njnt),
                        jsolimp = B.f("jnt_solimp", 5 * njnt);
    trn = B.ids("actuator_trnid", nu, nv);
    std::vector<int> dbody = B.i("dof_bodyid", nv);
    std::vector<double> floss = B.f("dof_frictionloss", nv), arm = B.f("dof_armature", nv), damp = B.f("dof_damping", nv),
                        diw = B.f("dof_invweight0", nv), dsolref = B.f("dof_solref", 2 * nv), dsolimp = B.f("dof_solimp", 5 * nv);
    std::vector<int> climited = B.i("actuator_ctrllimited", nu), flimited = B.i("actuator_forcelimited", nu);
    std::vector<double> gain = B.f("actuator_gainprm", 3 * nu), gear = B.f("actuator_gear", nu), bias = B.f("actuator_biasprm", 3 * nu),
                        crange = B.f("actuator_ctrlrange", 2 * nu), frange = B.f("actuator_forcerange", 2 * nu);
    if (int rc = reads_ok()) return rc;
    for (int t : jtype) if (t != JNT_HINGE && t != JNT_SLIDE) return fail(AW_EUNSUPPORTED, "joint type");
    PUT(jnt_type, jtype); PUT(jnt_bodyid, jbody); PUT(jnt_limited, jlim);
    PUT(jnt_pos, tof(jpos)); PUT(jnt_axis, tof(jaxis));
    PUT(jnt_range, tof(jrange)); PUT(jnt_margin, tof(jmargin));
    PUT(jnt_solref, tof(jsolref)); PUT(jnt_solimp, tof(jsolimp));
    PUT(jnt_range64, jrange); PUT(jnt_margin64, jmargin);
    PUT(jnt_pos64, jpos); PUT(jnt_axis64, jaxis);

    // actuators (joint transmission, one per dof)
    std::vector<int> dact(nv, -1);
    for (int u = 0; u < nu; u++) {
      if (dact[trn[u]] >= 0) return fail(AW_EUNSUPPORTED, "two actuators on one joint");
      dact[trn[u]] = u;
    }
    std::vector<int> fl_dof, fl_row(nv, -1);
    for (int j = 0; j < nv; j++)
      if (floss[j] > 0) { fl_row[j] = (int)fl_dof.size(); fl_dof.push_back(j); }
    m.nfl = (int)fl_dof.size();
    PUT(dof_bodyid, dbody); PUT(dof_act, dact); PUT(fl_dof, fl_dof);
    PUT(fl_row, fl_row);
    PUT(dof_armature, tof(arm)); PUT(dof_damping, tof(damp));
    PUT(dof_frictionloss, tof(floss)); PUT(dof_invweight0, tof(diw));
    PUT(dof_solref, tof(dsolref)); PUT(dof_solimp, tof(dsolimp));

    std::vector<float> g0(nu);
    for (int u = 0; u < nu; u++) g0[u] = (float)gain[3 * u];
    PUT(act_ctrllimited, climited); PUT(act_forcelimited, flimited);
    PUT(act_gear, tof(gear)); PUT(act_gain, g0);
    PUT(act_bias, tof(bias)); PUT(act_ctrlrange, tof(crange));
    PUT(act_forcerange, tof(frange));
    return AW_OK;
  }

  // compact collidable geoms
  int geoms_and_sites() {
    gtype = B.i("geom_type", ngeom_all); gbody = B.ids("geom_bodyid", ngeom_all, nbody);
    std::vector<int> gcon = B.i("geom_contype", ngeom_all), gaff = B.i("geom_conaffinity", ngeom_all);
    gpos = B.f("geom_pos", 3 * ngeom_all); gquat = B.f("geom_quat", 4 * ngeom_all); gsize = B.f("geom_size", 3 * ngeom_all);
    grb = B.f("geom_rbound", ngeom_all);
    sbody = B.ids("site_bodyid", nsite, nbody); spos = B.f("site_pos", 3 * nsite); squat = B.f("site_quat", 4 * nsite);
    if (int rc = reads_ok()) return rc;
    gmap.assign(ngeom_all, -1);
    std::vector<float> cpos, cquat, csize;
    std::vector<double> cpos64, cquat64, csize64;
    for (int g = 0; g < ngeom_all; g++) {
      if (gtype[g] == 7 || (gcon[g] == 0 && gaff[g] == 0)) continue;
      gmap[g] = (int)ctype.size();
      ctype.push_back(gtype[g]); cbody.push_back(gbody[g]);
      for (int k = 0; k < 3; k++) { cpos.push_back((float)gpos[3 * g + k]); csize.push_back((float)gsize[3 * g + k]); }
      for (int k = 0; k < 4; k++) cquat.push_back((float)gquat[4 * g + k]);
      for (int k = 0; k < 3; k++) { cpos64.push_back(gpos[3 * g + k]); csize64.push_back(gsize[3 * g + k]); }
      for (int k = 0; k < 4; k++) cquat64.push_back(gquat[4 * g + k]);
      crb.push_back((float)grb[g]);
    }
    PUT(geom_pos64, cpos64); PUT(geom_quat64, cquat64); PUT(geom_size64, csize64);
    m.ngeom = (int)ctype.size();
    if (m.ngeom > MAXG) return fail(AW_EUNSUPPORTED, "too many collidable geoms");
    memset(&data, 0, sizeof(data));   // stage_data's table: off, and the model geom id of each collidable geom
    for (int g = 0; g < ngeom_all; g++)
      if (gmap[g] >= 0) data.geom_id[gmap[g]] = g;
    PUT(geom_type, ctype); PUT(geom_bodyid, cbody); PUT(geom_pos, cpos);
    PUT(geom_quat, cquat); PUT(geom_size, csize); PUT(geom_rbound, crb);

    PUT(site_bodyid, sbody); PUT(site_pos, tof(spos));
    PUT(site_quat, tof(squat));
    return AW_OK;
  }

  // tendons: fixed, <= 2 joints
  int tendons() {
    std::vector<int> tadr = B.i("tendon_adr", ntendon), tnum = B.i("tendon_num", ntendon), wj = B.i("wrap_jnt");
    const int nwrap = (int)wj.size();
    std::vector<double> wc = B.f("wrap_coef", nwrap), tfl = B.f("tendon_frictionloss", ntendon);
    std::vector<int> tlimited = B.i("tendon_limited", ntendon);
    std::vector<double> trange = B.f("tendon_range", 2 * ntendon), tmargin = B.f("tendon_margin", ntendon),
                        tsolref = B.f("tendon_solref", 2 * ntendon), tsolimp = B.f("tendon_solimp", 5 * ntendon),
                        tiw = B.f("tendon_invweight0", ntendon);
    if (int rc = reads_ok()) return rc;
    std::vector<int> d0(ntendon), d1(ntendon);
    std::vector<float> c0(ntendon), c1(ntendon);
    std::vector<double> a0(ntendon), a1(ntendon);
    for (int t = 0; t < ntendon; t++) {
      if (tnum[t] < 1 || tnum[t] > 2) return fail(AW_EUNSUPPORTED, "tendon with != 1..2 joints");
      if (tfl[t] > 0) return fail(AW_EUNSUPPORTED, "tendon frictionloss");
      if (tadr[t] < 0 || tadr[t] + tnum[t] > nwrap) return fail(AW_EBLOB, "tendon_adr + tendon_num exceeds the wrap arrays");
      d0[t] = wj[tadr[t]]; c0[t] = (float)wc[tadr[t]];
      d1[t] = tnum[t] > 1 ? wj[tadr[t] + 1] : -1; c1[t] = tnum[t] > 1 ? (float)wc[tadr[t] + 1] : 0.f;
      if (d0[t] < 0 || d0[t] >= nv || d1[t] < -1 || d1[t] >= nv) return fail(AW_EBLOB, "wrap_jnt: joint of a tendon out of range");
      a0[t] = wc[tadr[t]]; a1[t] = tnum[t] > 1 ? wc[tadr[t] + 1] : 0.0;
    }
    PUT(ten_d0, d0); PUT(ten_d1, d1); PUT(ten_limited, tlimited);
    PUT(ten_c0, c0); PUT(ten_c1, c1); PUT(ten_range, tof(trange));
    PUT(ten_margin, tof(tmargin)); PUT(ten_solref, tof(tsolref));
    PUT(ten_solimp, tof(tsolimp)); PUT(ten_invweight0, tof(tiw));
    PUT(ten_range64, trange); PUT(ten_margin64, tmargin);
    PUT(ten_c0_64, a0); PUT(ten_c1_64, a1);
    return AW_OK;
  }

  // unified pair list: explicit pairs (own params), then candidates (params mixed here in fp64,
  // mj_contactParam with equal priorities)
  int pair_params() {
    std::vector<int> pcd;
    std::vector<float> pfr, psr, psi, pgp;
    std::vector<double> pmg64;
    std::vector<int> e1 = B.ids("pair_geom1", npair, ngeom_all), e2 = B.ids("pair_geom2", npair, ngeom_all),
                     ecd = B.i("pair_condim", npair);
    std::vector<double> efr = B.f("pair_friction", 5 * npair), esr = B.f("pair_solref", 2 * npair),
                        esi = B.f("pair_solimp", 5 * npair), emg = B.f("pair_margin", npair), egp = B.f("pair_gap", npair);
    std::vector<int> c1v = B.ids("cand_geom1", ncand, ngeom_all), c2v = B.ids("cand_geom2", ncand, ngeom_all),
                     gcd = B.i("geom_condim", ngeom_all);
    std::vector<double> gfr = B.f("geom_friction", 3 * ngeom_all), gsm = B.f("geom_solmix", ngeom_all),
                        gsr = B.f("geom_solref", 2 * ngeom_all), gsi = B.f("geom_solimp", 5 * ngeom_all),
                        gmg = B.f("geom_margin", ngeom_all), ggp = B.f("geom_gap", ngeom_all);
    if (int rc = reads_ok()) return rc;
    for (int p = 0; p < npair; p++) {
      if (gmap[e1[p]] < 0 || gmap[e2[p]] < 0) return fail(AW_EUNSUPPORTED, "pair with a visual geom");
      pg1.push_back(gmap[e1[p]]); pg2.push_back(gmap[e2[p]]); pcd.push_back(ecd[p]);
      for (int k = 0; k < 5; k++) pfr.push_back((float)efr[5 * p + k]);
      for (int k = 0; k < 2; k++) psr.push_back((float)esr[2 * p + k]);
      for (int k = 0; k < 5; k++) psi.push_back((float)esi[5 * p + k]);
      pmg.push_back((float)emg[p]); pgp.push_back((float)egp[p]); pmg64.push_back(emg[p]);
    }
    for (int c = 0; c < ncand; c++) {
      int a = c1v[c], b = c2v[c];
      if (gmap[a] < 0 || gmap[b] < 0) return fail(AW_EBLOB, "collision candidate with a visual geom");
      pg1.push_back(gmap[a]); pg2.push_back(gmap[b]);
      pcd.push_back(std::max(gcd[a], gcd[b]));
      double s1 = gsm[a], s2 = gsm[b], mix;
      if (s1 >= 1e-15 && s2 >= 1e-15) mix = s1 / (s1 + s2);
      else if (s1 < 1e-15 && s2 < 1e-15) mix = 0.5;
      else mix = s1 < 1e-15 ? 0.0 : 1.0;
      double f0 = std::max(gfr[3 * a], gfr[3 * b]), f1 = std::max(gfr[3 * a + 1], gfr[3 * b + 1]),
             f2 = std::max(gfr[3 * a + 2], gfr[3 * b + 2]);
      double fr[5] = {f0, f0, f1, f2, f2};
      for (int k = 0; k < 5; k++) pfr.push_back((float)fr[k]);
      for (int k = 0; k < 2; k++) psr.push_back((float)(mix * gsr[2 * a + k] + (1 - mix) * gsr[2 * b + k]));
      for (int k = 0; k < 5; k++) psi.push_back((float)(mix * gsi[5 * a + k] + (1 - mix) * gsi[5 * b + k]));
      pmg.push_back((float)std::max(gmg[a], gmg[b])); pgp.push_back((float)std::max(ggp[a], ggp[b]));
      pmg64.push_back(std::max(gmg[a], gmg[b]));
    }
    m.npairall = (int)pg1.size();
    if (m.npairall > JL * VS * 2) return fail(AW_EUNSUPPORTED, "too many collision pairs");
    PUT(cp_margin64, pmg64);
    PUT(cp_g1, pg1); PUT(cp_g2, pg2); PUT(cp_condim, pcd); PUT(cp_friction, pfr);
    PUT(cp_solref, psr); PUT(cp_solimp, psi); PUT(cp_margin, pmg); PUT(cp_gap, pgp);
    return AW_OK;
  }

  // per pair: collider class, broadphase radius, fp64 frame masks and the bodies' row data
  int pair_classes() {
    // collider class per pair (aw_collide.h collide_pair dispatch) and the broadphase radius
    std::vector<int> pcls(m.npairall);
    std::vector<float> prb(m.npairall);
    int ccount[NCLASS] = {0, 0, 0, 0, 0};
    for (int p = 0; p < m.npairall; p++) {
      int a = pg1[p], b = pg2[p];
      int ta = ctype[a], tb = ctype[b];
      int lo = std::min(ta, tb), hi = std::max(ta, tb);
      int c;
      if (lo == GEOM_PLANE) c = 0;
      else if (lo == GEOM_CYLINDER || hi == GEOM_CYLINDER) c = 4;
      else if (hi == GEOM_BOX && lo == GEOM_BOX) c = 3;
      else if (hi == GEOM_BOX) c = 2;
      else c = 1;
      pcls[p] = c;
      ccount[c]++;
      // plane pairs: -(1 + rbound of the other geom + margin) (< -1: the broadphase's plane test)
      prb[p] = lo == GEOM_PLANE ? (float)(-1.0 - (double)crb[ta == GEOM_PLANE ? b : a] - (double)pmg[p])
                                : (float)((double)crb[a] + (double)crb[b] + (double)pmg[p]);
    }
    m.cls_start[0] = 0;
    for (int c = 0; c < NCLASS; c++) m.cls_start[c + 1] = m.cls_start[c] + ccount[c];
    PUT(cp_class, pcls); PUT(cp_rb, prb);
    // per pair: the bodies whose fp64 frames its geometry needs (stage_kin64), with ancestors
    // (every class: the sphere / capsule pairs' near-margin contacts are decided on fp64 frames too)
    std::vector<unsigned long long> k64(m.npairall, 0ull);
    for (int p = 0; p < m.npairall; p++)
      for (int g : {pg1[p], pg2[p]})
        for (int b = cbody[g]; b > 0; b = parent[b]) k64[p] |= 1ull << b;
    PUT(cp_kin64, k64);
    std::vector<int> ppack(m.npairall);
    for (int p = 0; p < m.npairall; p++) ppack[p] = pcls[p] | (pg1[p] << 8) | (pg2[p] << 16);
    PUT(cp_pack, ppack);

    std::vector<double> iw = B.f("body_invweight0", 2 * nbody);
    if (int rc = reads_ok()) return rc;
    std::vector<float> ptran(pg1.size()), prot(pg1.size());
    std::vector<int> pr1(pg1.size()), pr2(pg1.size());
    std::vector<unsigned long long> pm1(pg1.size()), pm2(pg1.size());
    for (size_t p = 0; p < pg1.size(); p++) {
      const int b1 = cbody[pg1[p]], b2 = cbody[pg2[p]];
      ptran[p] = (float)iw[2 * b1] + (float)iw[2 * b2];
      prot[p] = (float)iw[2 * b1 + 1] + (float)iw[2 * b2 + 1];
      pr1[p] = rootid[b1]; pr2[p] = rootid[b2];
      pm1[p] = bmask[b1]; pm2[p] = bmask[b2];
    }
    PUT(cp_tran, ptran); PUT(cp_rot, prot); PUT(cp_root1, pr1); PUT(cp_root2, pr2);
    PUT(cp_mask1, pm1); PUT(cp_mask2, pm2);
    return AW_OK;
  }

  // task block: object ids, and the object each per-env param overrides (a geom: its collidable index)
  int task_block() {
    tidx = B.i("task_idx"); pf = B.i("task_param_field", m.nparam); po = B.i("task_param_obj", m.nparam);
    pc = B.i("task_param_comp", m.nparam);
    if (int rc = reads_ok()) return rc;
    for (int p = 0; p < m.nparam; p++) {
      const int f = pf[p];
      const int lim = (f == 0 || f == 1 || f == 3) ? nbody : f == 2 ? nsite : (f == 4 || f == 5) ? ngeom_all : -1;
      if (lim >= 0 && (po[p] < 0 || po[p] >= lim)) return fail(AW_EBLOB, "task_param_obj out of range for its field");
      if (f == 4 || f == 5) {
        if (gmap[po[p]] < 0) return fail(AW_EUNSUPPORTED, "param on a visual geom");
        po[p] = gmap[po[p]];
      }
    }
    PUT(task_idx, tidx); PUT(param_field, pf); PUT(param_obj, po); PUT(param_comp, pc);
    return AW_OK;
  }

  // every sensor in MuJoCo's order (stage_sensors): one scalar each, so nsensordata = nsensor
  int sensor_table() {
    if (nsensor > MAXSENS) return fail(AW_EUNSUPPORTED, "more sensors than MAXSENS");
    if (nsensor > 0) {
      stype = B.i("sensor_type", nsensor); sobj = B.i("sensor_objid", nsensor); sadr = B.i("sensor_adr", nsensor);
    }
    if (B.has("site_type")) sitetype = B.i("site_type", nsite);
    if (B.has("site_size")) ssize = B.f("site_size", 3 * nsite);
    if (int rc = reads_ok()) return rc;
    for (int k = 0; k < nsensor; k++) {
      const int lim = stype[k] == SENS_TOUCH ? nsite : stype[k] == SENS_JOINTPOS ? njnt
                      : stype[k] == SENS_ACTUATORFRC ? nu : -1;
      if (lim < 0) return fail(AW_EUNSUPPORTED, "sensor type (touch, jointpos and actuatorfrc are supported)");
      if (sobj[k] < 0 || sobj[k] >= lim || sadr[k] < 0 || sadr[k] >= nsensor) return fail(AW_EBLOB, "sensor object / address out of range");
    }
    if (nsensor > 0 && !(B.has("site_type") && B.has("site_size"))) return fail(AW_EBLOB, "model table lacks the site shapes");
    sens.n = nsensor;
    sens.out = nullptr;
    if (!put_arr(sens.type, stype) || !put_arr(sens.obj, sobj) || !put_arr(sens.adr, sadr) || !put_arr(sens.act_dof, trn) ||
        !put_arr(sens.site_type, sitetype) || !put_arr(sens.site_size, tof(ssize)))
      return fail(AW_EUNSUPPORTED, "sensor tables exceed kernel capacity");
    return AW_OK;
  }

  // touch sensors read by the task (hammer: S_nail, task_idx[5] = its sensordata address)
  int touch_pads() {
    std::vector<int> ts, ttype;
    std::vector<float> tsize;
    if (m.task_kind == 0 && tidx.size() > 5)
      for (int k = 0; k < nsensor; k++)
        if (sadr[k] == tidx[5] && stype[k] == 0) {
          ts.push_back(sobj[k]); ttype.push_back(sitetype[sobj[k]]);
          for (int q = 0; q < 3; q++) tsize.push_back((float)ssize[3 * sobj[k] + q]);
        }
    m.ntouch = (int)ts.size();
    PUT(touch_site, ts); PUT(touch_adr, ts); PUT(touch_type, ttype); PUT(touch_size, tsize);
    return AW_OK;
  }

  // depth renderer: every primitive (non-mesh) geom in model order
  int render_table() {
    for (int g = 0; g < ngeom_all; g++) {
      if (gtype[g] == 7) continue;
      rt.push_back(gtype[g]); rb.push_back(gbody[g]); rc.push_back(gmap[g]);
      for (int k = 0; k < 3; k++) { rp.push_back(gpos[3 * g + k]); rs.push_back(gsize[3 * g + k]); }
      for (int k = 0; k < 4; k++) rq.push_back(gquat[4 * g + k]);
      rr.push_back(grb[g]);
    }
    m.nrgeom = (int)rt.size();
    rsite.assign(rt.size(), -1);
    // colour renderer: the visible sites (group 0-2, alpha > 0) follow the geoms, then every
    // entry's colour record.  A model table without the appearance arrays renders depth only.
    m.appearance = B.has("geom_rgba") && B.has("geom_group") && B.has("geom_matid") && B.has("site_rgba") &&
                   B.has("site_group") && B.has("site_matid") && B.has("site_type") && B.has("site_size") &&
                   B.has("mat_rgba") && B.has("light_pos");
    return AW_OK;
  }

  // the colour record of every render entry; the visible sites join the table here
  int colours() {
    if (!m.appearance) return AW_OK;
    std::vector<double> mspec = B.f("mat_specular");
    const int nmat = (int)mspec.size();
    std::vector<double> grgba = B.f("geom_rgba", 4 * ngeom_all), srgba = B.f("site_rgba", 4 * nsite), mrgba = B.f("mat_rgba", 4 * nmat),
                        mshin = B.f("mat_shininess", nmat), memi = B.f("mat_emission", nmat);
    std::vector<int> ggroup = B.i("geom_group", ngeom_all), gmat = B.i("geom_matid", ngeom_all), sgroup = B.i("site_group", nsite),
                     smat = B.i("site_matid", nsite);
    if (int rc = reads_ok()) return rc;
    // rgb: an explicit rgba, else the material's (MuJoCo: a geom rgba left at its default
    // 0.5 0.5 0.5 1 yields to the material); alpha as written
    auto record = [&](int src_mat, const double* src_rgba, double alpha) {
      const bool dflt = src_rgba[0] == 0.5 && src_rgba[1] == 0.5 && src_rgba[2] == 0.5 && src_rgba[3] == 1.0;
      const double* c = (src_mat >= 0 && dflt) ? &mrgba[4 * src_mat] : src_rgba;
      for (int k = 0; k < 3; k++) rcol.push_back((float)c[k]);
      rcol.push_back((float)alpha);
      rcol.push_back((float)(src_mat >= 0 ? mspec[src_mat] : 0.5));
      rcol.push_back((float)(128.0 * (src_mat >= 0 ? mshin[src_mat] : 0.5)));
      rcol.push_back((float)(src_mat >= 0 ? memi[src_mat] : 0.0));
      rcol.push_back(0.f);
    };
    for (int g = 0; g < ngeom_all; g++) {
      if (gtype[g] == 7) continue;
      if (gmat[g] >= nmat) return fail(AW_EBLOB, "geom material id out of range");
      // stand-in rule: a primitive in a group hidden by default (>= 3) is drawn in place of its
      // body's mesh (absent), with the first mesh geom's colour and material; geoms are opaque
      int src = g;
      if (ggroup[g] >= 3)
        for (int q = 0; q < ngeom_all; q++)
          if (gtype[q] == 7 && gbody[q] == gbody[g]) { src = q; break; }
      if (gmat[src] >= nmat) return fail(AW_EBLOB, "geom material id out of range");
      record(gmat[src], &grgba[4 * src], 1.0);
    }
    for (int i = 0; i < nsite; i++) {
      if (sgroup[i] > 2 || !(srgba[4 * i + 3] > 0)) continue;
      if (smat[i] >= nmat) return fail(AW_EBLOB, "site material id out of range");
      rt.push_back(sitetype[i]); rb.push_back(sbody[i]); rc.push_back(-1); rsite.push_back(i);
      for (int k = 0; k < 3; k++) { rp.push_back(spos[3 * i + k]); rs.push_back(ssize[3 * i + k]); }
      for (int k = 0; k < 4; k++) rq.push_back(squat[4 * i + k]);
      const double* z = &ssize[3 * i];
      const int st = sitetype[i];
      rr.push_back(st == GEOM_SPHERE ? z[0] : st == GEOM_CAPSULE ? z[0] + z[1]
                   : st == GEOM_CYLINDER ? std::sqrt(z[0] * z[0] + z[1] * z[1])
                   : st == GEOM_BOX ? std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) : 0.0);
      record(smat[i], &srgba[4 * i], srgba[4 * i + 3]);
    }
    m.nrsite = (int)rt.size() - m.nrgeom;
    if ((int)rt.size() > MAXRG) return fail(AW_EBLOB, "more render entries (primitive geoms + visible sites) than MAXRG");
    return AW_OK;
  }

  // lights and the task block's tint rows, then the finished render table
  int lights_and_tints() {
    if (m.appearance) {
      // lights: positional lights with a cutoff below 180 degrees carry cos(cutoff), the others -2
      std::vector<double> lcut = B.f("light_cutoff");
      m.nlight = (int)lcut.size();
      if (m.nlight > MAXLIGHT) return fail(AW_EBLOB, "more lights than MAXLIGHT");
      const int nl = m.nlight;
      std::vector<double> lpos = B.f("light_pos", 3 * nl), ldir = B.f("light_dir", 3 * nl), lamb = B.f("light_ambient", 3 * nl),
                          ldif = B.f("light_diffuse", 3 * nl), lspe = B.f("light_specular", 3 * nl),
                          latt = B.f("light_attenuation", 3 * nl), lexp = B.f("light_exponent", nl);
      std::vector<int> ldirl = B.i("light_directional", nl);
      // tint rows of the task block
      std::vector<double> tscale = B.f("task_tint_scale");
      m.ntint = (int)tscale.size();
      std::vector<int> tint = B.i("task_tint");
      if (int rc = reads_ok()) return rc;
      std::vector<float> lrec;
      for (int l = 0; l < nl; l++) {
        for (const std::vector<double>* v : {&lpos, &ldir, &lamb, &ldif, &lspe, &latt})
          for (int k = 0; k < 3; k++) lrec.push_back((float)(*v)[3 * l + k]);
        lrec.push_back(!ldirl[l] && lcut[l] < 180.0 ? (float)std::cos(lcut[l] * 3.14159265358979323846 / 180.0) : -2.f);
        lrec.push_back((float)lexp[l]);
        lrec.push_back(ldirl[l] ? 1.f : 0.f);
        lrec.resize((size_t)(l + 1) * LIGHT_W, 0.f);
      }
      PUT(light, lrec);
      if (m.ntint > MAXTINT || (int)tint.size() != 3 * m.ntint) return fail(AW_EBLOB, "bad tint rows");
      std::vector<int> te, tc, tsl;
      for (int t = 0; t < m.ntint; t++) {
        if (tint[3 * t] < 0 || tint[3 * t] >= (int)rt.size() || tint[3 * t + 1] < 0 || tint[3 * t + 1] > 2 ||
            tint[3 * t + 2] < 0 || tint[3 * t + 2] >= m.nparam)
          return fail(AW_EBLOB, "tint row out of range");
        te.push_back(tint[3 * t]); tc.push_back(tint[3 * t + 1]); tsl.push_back(tint[3 * t + 2]);
      }
      PUT(tint_entry, te); PUT(tint_chan, tc); PUT(tint_slot, tsl); PUT(tint_scale, tof(tscale));
    }
    PUT(rg_type, rt); PUT(rg_body, rb); PUT(rg_cgeom, rc); PUT(rg_pos, rp); PUT(rg_quat, rq);
    PUT(rg_size, rs); PUT(rg_rbound, rr); PUT(rg_site, rsite); PUT(rg_col, rcol);
    return AW_OK;
  }

  // per-object "some parameter overrides this" flags (kinematics applies those overrides inline),
  // the action scaling, the params' defaults and their reset draws
  int overrides_and_draws() {
    std::vector<int> bo(nbody, 0), so(std::max(nsite, 1), 0), go(std::max(m.ngeom, 1), 0);
    for (int p = 0; p < m.nparam; p++) {
      if (pf[p] == 0 || pf[p] == 1 || pf[p] == 3) bo[po[p]] = 1;
      else if (pf[p] == 2) so[po[p]] = 1;
      else if (pf[p] == 4 || pf[p] == 5) go[po[p]] = 1;
    }
    PUT(body_ovr, bo); PUT(site_ovr, so); PUT(geom_ovr, go);
    std::vector<double> amid = B.f("task_act_mid", nu), arng = B.f("task_act_rng", nu);
    std::vector<int> pdraw = B.i("task_param_draw", m.nparam);
    std::vector<double> dlo = B.f("task_draw_lo");
    m.ndraw = (int)dlo.size();
    std::vector<double> dhi = B.f("task_draw_hi", m.ndraw);
    std::vector<float> pdef;
    if (int rc = param_defaults(B, m.nparam, pdef, err)) return rc;
    PUT(act_mid, tof(amid)); PUT(act_rng, tof(arng));
    PUT(param_default, pdef);
    PUT(param_draw, pdraw);
    if (m.ndraw > 8) return fail(AW_EUNSUPPORTED, "too many reset draws");
    PUT(draw_lo, tof(dlo)); PUT(draw_hi, tof(dhi));
    return AW_OK;
  }
};
#undef PUT

// the model table -> the device tables (host copies; aw_create uploads them)
inline int build_model(const Blob& B, DModel& m, MData& md, SensTab& sens, DataTab& data, std::string& err) {
  ModelBuild b{B, m, md, sens, data, err};
  return b.run();
}

// the model's dof tree must be the compiled one of its task (aw_trees.h, tools/gen_trees.py)
template <int TASK>
bool tree_matches(const std::vector<int>& par) {
  if ((int)par.size() != TreeDef<TASK>::NV) return false;
  for (int j = 0; j < TreeDef<TASK>::NV; j++)
    if (par[j] != TreeDef<TASK>::parent[j]) return false;
  return true;
}
inline int check_tree(const Blob& B, int task_kind, std::string& err) {
  const std::vector<int> par = B.i("dof_parentid");
  bool ok = false;
  switch (task_kind) {
    case 0: ok = tree_matches<0>(par); break;
    case 1: ok = tree_matches<1>(par); break;
    case 2: ok = tree_matches<2>(par); break;
    case 3: ok = tree_matches<3>(par); break;
    default: err = "unknown task kind"; return AW_EUNSUPPORTED;
  }
  if (!ok) {
    err = "model dof tree differs from the compiled tree of its task "
          "(mj_envs_amd/csrc/aw_trees.h: run tools/gen_trees.py and rebuild)";
    return AW_EUNSUPPORTED;
  }
  return AW_OK;
}

// ... and so must the built table's ancestor masks: stage_crb takes the structure of M from the
// compiled tree (AW_CRB_TREE) while the solver stages read dof_ancmask, and the two must describe
// one tree.  The masks are compared bit for bit, rows past nv included (they must be empty).
template <int TASK>
bool ancmask_matches(const MData& md) {
  for (int j = 0; j < MAXV; j++) {
    unsigned long long want = 0;
    if (j < TreeDef<TASK>::NV)
      for (int p = TreeDef<TASK>::parent[j]; p >= 0; p = TreeDef<TASK>::parent[p]) want |= 1ull << p;
    if (md.dof_ancmask[j] != want) return false;
  }
  return true;
}
inline int check_tree(const Blob& B, int task_kind, const MData& md, std::string& err) {
  if (int rc = check_tree(B, task_kind, err)) return rc;
  bool ok = false;
  switch (task_kind) {
    case 0: ok = ancmask_matches<0>(md); break;
    case 1: ok = ancmask_matches<1>(md); break;
    case 2: ok = ancmask_matches<2>(md); break;
    case 3: ok = ancmask_matches<3>(md); break;
  }
  if (!ok) {
    err = "model table's dof_ancmask differs from the compiled dof tree of its task "
          "(mj_envs_amd/csrc/aw_trees.h: run tools/gen_trees.py and rebuild)";
    return AW_EUNSUPPORTED;
  }
  return AW_OK;
}

}  // namespace aw
