// Test hooks of the non-GEMM kernels of the VAE path (include/sln_hip.h, sln_debug_vae_*): plain-C descriptions in, the launchers
// of vae_kernels.h / vae_multi.h out.  No kernel lives here; what a hook refuses is what the launchers assume by construction.
#include <cstdint>
#include <cstring>
#include <vector>
#include "sln_debug.h"
#include "vae_multi.h"

namespace {

bool dbg_csr(const SlnDbgCsr& d, GraphCsr& g) {
  std::memset(&g, 0, sizeof(g));
  if (d.T < 0 || d.O < 1 || !d.deg || !d.invdeg || !d.rowptr || !d.cursor) return false;
  if (d.T > 0 && (!d.s || !d.p || !d.o || !d.ent)) return false;
  g.s = d.s; g.p = d.p; g.o = d.o; g.deg = d.deg; g.invdeg = d.invdeg; g.rowptr = d.rowptr; g.cursor = d.cursor; g.ent = d.ent;
  g.T = d.T; g.O = d.O;
  return true;
}

// the statistics of a view span `cols` columns
bool dbg_fwd_bn(const SlnDbgBn& d, int cols, BnView& v) {
  if (!sln_dbg_bn(d, SLN_COEF_FWD, v)) return false;
  return d.mode != SLN_BN_TRAIN || d.cstride >= cols;
}

enum { E_SCATTER_FWD = 0, E_SCATTER_BWD = 1, E_GATHER_BWD = 2, E_MASK_GSTATS = 3, E_BN_RELU = 4, E_ADD2 = 5 };

bool dbg_edge_ok(const SlnDbgEdge& d, GraphCsr& g, BnView& bn) {
  std::memset(&g, 0, sizeof(g));
  std::memset(&bn, 0, sizeof(bn));
  if (!d.a || !d.out || d.rows < 1) return false;
  switch (d.kind) {
    case E_SCATTER_FWD:
      return d.H > 0 && d.D > 0 && d.lda >= 2 * d.H + d.D && dbg_csr(d.g, g) && d.rows == g.O && dbg_fwd_bn(d.bn, 2 * d.H + d.D, bn);
    case E_SCATTER_BWD:
      return d.H > 0 && d.D > 0 && d.c && d.ldc >= 2 * d.H + d.D && dbg_csr(d.g, g) && d.rows == g.T &&
             (!d.b || (d.col0 >= 0 && d.ldb >= d.col0 + d.D)) && (!d.gsums || d.cstride >= 2 * d.H + d.D) && dbg_fwd_bn(d.bn, 2 * d.H + d.D, bn);
    case E_GATHER_BWD:
      if (!(d.D > 0 && d.lda >= 3 * d.D && d.ldo >= d.D && dbg_csr(d.g, g) && d.rows == g.O && (!d.b || d.ldb >= d.D))) return false;
      if (!d.masked) return true;
      return d.c && d.ldc >= d.D && (!d.gsums || d.cstride >= d.D) && dbg_fwd_bn(d.bn, d.D, bn);
    case E_MASK_GSTATS:
      return d.cols > 0 && d.c && d.lda >= d.cols && d.ldc >= d.cols && d.ldo >= d.cols && (!d.b || d.ldb >= d.cols) &&
             (!d.gsums || d.cstride >= d.cols) && dbg_fwd_bn(d.bn, d.cols, bn);
    case E_BN_RELU:
      return d.cols > 0 && d.col0 >= 0 && d.lda >= d.col0 + d.cols && d.ldo >= d.cols && dbg_fwd_bn(d.bn, d.cols, bn);
    case E_ADD2:
      return d.cols > 0 && d.b && d.lda >= d.cols && d.ldb >= d.cols && d.ldo >= d.cols;
  }
  return false;
}

int edge_single(const SlnDbgEdge& d, const GraphCsr& g, const BnView& bn, hipStream_t st) {
  switch (d.kind) {
    case E_SCATTER_FWD: return sln_launch_scatter_avg_fwd(d.a, d.lda, d.H, d.D, bn, g, d.rows, d.out, st);
    case E_SCATTER_BWD: return sln_launch_scatter_avg_bwd(d.a, d.b, d.ldb, d.col0, d.c, d.ldc, d.H, d.D, bn, g, d.rows, d.out, d.gsums, d.cstride, st);
    case E_GATHER_BWD:
      return sln_launch_gather_bwd(d.a, d.lda, d.D, g, d.rows, d.b, d.ldb, d.c, d.ldc, bn, d.masked, d.out, d.ldo, d.gsums, d.cstride, st);
    case E_MASK_GSTATS: return sln_launch_mask_gstats(d.a, d.lda, d.b, d.ldb, d.c, d.ldc, bn, d.rows, d.cols, d.out, d.ldo, d.gsums, d.cstride, st);
    case E_BN_RELU: return sln_launch_bn_relu_apply(d.a, d.lda, d.col0, d.cols, d.rows, bn, d.out, d.ldo, st);
    default: return sln_launch_add2(d.a, d.lda, d.b, d.ldb, d.rows, d.cols, d.out, d.ldo, st);
  }
}

// a host table on the device for the length of one launch
template <typename T>
struct DevTable {
  T* p = nullptr;
  int upload(const std::vector<T>& h) {
    int r = (int)hipMalloc((void**)&p, sizeof(T) * h.size());
    if (!r) r = (int)hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice);
    return r;
  }
  int finish(int r, hipStream_t st) {            // the table must outlive the launch
    const int rs = (int)hipStreamSynchronize(st);
    if (p) (void)hipFree(p);
    p = nullptr;
    return r ? r : rs;
  }
};

// plan every room, refuse mixed variants, one launch over the largest per-room grid
template <typename M> auto room_gy(const M& m, int) -> decltype(m.gy) { return m.gy; }
template <typename M> int room_gy(const M&, long) { return 1; }
template <typename M, typename Plan, typename Launch>
int edge_multi(std::vector<M>& rooms, Plan plan, Launch launch, int* variant, hipStream_t st) {
  int var = -1, gx = 0, gy = 0;
  for (size_t i = 0; i < rooms.size(); ++i) {
    rooms[i].gx = 0;
    const int v = plan(rooms[i]);
    if (v < 0) return SLN_E_UNSUPPORTED;              // (-2 as well: what the single-room launcher answers)
    if (i > 0 && v != var) return SLN_E_UNSUPPORTED;
    var = v;
    gx = rooms[i].gx > gx ? rooms[i].gx : gx;
    gy = room_gy(rooms[i], 0) > gy ? room_gy(rooms[i], 0) : gy;
  }
  if (variant) *variant = var;
  DevTable<M> tab;
  int r = tab.upload(rooms);
  if (!r) r = launch(tab.p, (int)rooms.size(), var, gx, gy, st);
  return tab.finish(r, st);
}

enum { M_ENC = 0, M_ENC_BWD = 1, M_DEC = 2, M_DEC_BWD = 3, M_GATHER = 4, M_BWD_I32 = 5, M_BWD_I64 = 6, M_I64_I32 = 7, M_STAGE = 8, M_VALIDATE = 9 };

bool dbg_enc(const SlnDbgEmbed& d, EncAssemble& a) {
  if (d.O < 1 || d.n_obj < 1 || d.n_attr < 0 || d.n_box < 1 || d.n_angle < 1 || d.box_dim < 1 || d.box_dim > 6) return false;
  if (!d.objs || !d.angles || !d.boxes || !d.obj_emb || !d.angle_emb || !d.wb || !d.bb || !d.x0 || (d.n_attr > 0 && (!d.attrs || !d.attr_emb))) return false;
  a = EncAssemble{d.objs, d.attrs, d.angles, d.boxes, d.obj_emb, d.attr_emb, d.angle_emb, d.wb, d.bb, d.O, d.n_obj, d.n_attr, d.n_box, d.n_angle, d.box_dim, d.x0};
  return true;
}

bool dbg_embed_ok(const SlnDbgEmbed& d) {
  if (d.O < 1) return false;
  const bool attr = d.n_attr == 0 || (d.n_attr > 0 && d.attrs), rows = d.rows_obj >= 0 && d.rows_attr >= 0 && d.rows_angle >= 0;
  EncAssemble e;
  switch (d.kind) {
    case M_ENC: return dbg_enc(d, e);
    case M_ENC_BWD:
      return d.n_obj > 0 && d.n_box > 0 && d.n_angle > 0 && d.box_dim >= 1 && d.box_dim <= 6 && attr && rows && d.objs && d.angles && d.boxes && d.dx0 &&
             d.d_obj_emb && d.d_angle_emb && d.d_wb && d.d_bb && (d.n_attr == 0 || d.d_attr_emb);
    case M_DEC:
      return d.n_obj > 0 && d.n_z > 0 && attr && d.objs && d.obj_emb && (d.n_attr == 0 || d.attr_emb) && d.x0 &&
             (d.z_in || (d.mu && (d.use_ae || (d.logvar && d.eps))));
    case M_DEC_BWD:
      return d.n_obj > 0 && d.n_z >= 0 && (!d.z_in_x0 || d.n_z > 0) && attr && rows && d.objs && d.dx0 && d.d_obj_emb && (d.n_attr == 0 || d.d_attr_emb);
    case M_GATHER: return d.idx && d.src && d.dst && d.n > 0;
    case M_BWD_I32: case M_BWD_I64: return d.idx && d.src && d.dst && d.n > 0 && d.col0 >= 0 && d.ld >= d.col0 + d.n && d.table_rows >= 0;
    case M_I64_I32: return d.idx && d.dst;
    case M_STAGE:
      return d.objs && d.attrs && d.angles && d.boxes && d.st_objs && d.st_attrs && d.st_angles && d.st_boxes && d.attrs32 && d.deg && d.err &&
             d.box_dim > 0 && rows;
    case M_VALIDATE: return d.objs && d.attrs && d.err && rows;
  }
  return false;
}

DecAssemble dbg_dec(const SlnDbgEmbed& d) {
  return DecAssemble{d.objs, d.attrs, d.obj_emb, d.attr_emb, d.mu, d.logvar, d.eps, d.z_in, d.O, d.n_obj, d.n_attr, d.n_z, d.use_ae, d.z, d.x0, d.z_in_x0};
}
DecAssembleBwd dbg_dec_bwd(const SlnDbgEmbed& d) {
  return DecAssembleBwd{d.objs, d.attrs, d.dx0, d.O, d.n_obj, d.n_attr, d.n_z, d.d_obj_emb, d.d_attr_emb, d.dz, d.z_in_x0, d.rows_obj, d.rows_attr};
}

int embed_single(const SlnDbgEmbed& d, hipStream_t st) {
  switch (d.kind) {
    case M_ENC: { EncAssemble e; dbg_enc(d, e); return sln_launch_enc_assemble(e, st); }
    case M_ENC_BWD:
      return sln_launch_enc_assemble_bwd(EncAssembleBwd{d.objs, d.attrs, d.angles, d.boxes, d.dx0, d.O, d.n_obj, d.n_attr, d.n_box, d.n_angle, d.box_dim,
                                                        d.d_obj_emb, d.d_attr_emb, d.d_angle_emb, d.d_wb, d.d_bb, d.rows_obj, d.rows_attr, d.rows_angle}, st);
    case M_DEC: return sln_launch_dec_assemble(dbg_dec(d), st);
    case M_DEC_BWD: return sln_launch_dec_assemble_bwd(dbg_dec_bwd(d), st);
    case M_GATHER: return sln_launch_embed_gather_i32(static_cast<const int*>(d.idx), d.src, d.O, d.n, static_cast<float*>(d.dst), st);
    case M_BWD_I32: return sln_launch_embed_bwd_i32(static_cast<const int*>(d.idx), d.src, d.ld, d.col0, d.O, d.n, d.table_rows, static_cast<float*>(d.dst), st);
    case M_BWD_I64: return sln_launch_embed_bwd_i64(static_cast<const int64_t*>(d.idx), d.src, d.ld, d.col0, d.O, d.n, d.table_rows, static_cast<float*>(d.dst), st);
    case M_I64_I32: return sln_launch_i64_to_i32(static_cast<const int64_t*>(d.idx), static_cast<int*>(d.dst), d.O, st);
    case M_STAGE:
      return sln_launch_stage_batch(StageBatch{d.objs, d.attrs, d.angles, d.boxes, d.st_objs, d.st_attrs, d.st_angles, d.st_boxes, d.attrs32, d.deg, d.err,
                                               d.O, d.box_dim, d.rows_obj, d.rows_attr, d.rows_angle}, st);
    default: return sln_launch_validate_ids(d.objs, d.attrs, d.angles, d.O, d.rows_obj, d.rows_attr, d.rows_angle, d.err, st);
  }
}

// the decoder's assembled-input gradients: the planner writes each room's block into a blob (AssembleBwdLds is private to vae_kernels.hip)
int dec_bwd_multi(const SlnDbgEmbed* desc, int n, int* variant, hipStream_t st) {
  std::vector<char> blobs((size_t)n * SLN_ASM_BLOB);
  int var = -1, gx = 0, smem = 0;
  for (int i = 0; i < n; ++i) {
    int g = 0, f = 0;
    const int v = sln_plan_dec_assemble_bwd(dbg_dec_bwd(desc[i]), blobs.data() + (size_t)i * SLN_ASM_BLOB, &g, &f);
    if (v < 0 || (i > 0 && v != var)) return SLN_E_UNSUPPORTED;
    var = v; gx = g > gx ? g : gx; smem = f > smem ? f : smem;
  }
  if (variant) *variant = var;
  DevTable<char> tab;
  int r = tab.upload(blobs);
  if (!r) r = sln_launch_dec_assemble_bwd_multi(tab.p, n, var, gx, smem, st);
  return tab.finish(r, st);
}

}  // namespace

extern "C" int sln_debug_vae_sizes(int* out, int max) {
  const int sz[7] = {(int)sizeof(SlnDbgCsr), (int)sizeof(SlnDbgEdge), (int)sizeof(SlnDbgLoss), (int)sizeof(SlnDbgBnEntry),
                     (int)sizeof(SlnDbgTranspose), (int)sizeof(SlnDbgOpt), (int)sizeof(SlnDbgEmbed)};
  for (int i = 0; out && i < 7 && i < max; ++i) out[i] = sz[i];
  return 7;
}

extern "C" int sln_debug_vae_csr(const int64_t* triples, int num_preds, int edges_only, int deg_is_zero, const SlnDbgCsr* desc, int* err,
                                 void* stream) {
  GraphCsr g;
  if (!desc || !dbg_csr(*desc, g) || (g.T > 0 && !triples) || (!edges_only && num_preds < 1)) return SLN_E_BADARG;
  return sln_launch_graph_prep(triples, g.T, g.O, edges_only ? 1 : num_preds, g, err, (hipStream_t)stream, edges_only ? 1 : 0, deg_is_zero ? 1 : 0);
}

extern "C" int sln_debug_vae_edge(const SlnDbgEdge* desc, int n, int multi, int* variant, void* stream) {
  if (!desc || n < 1 || n > 64 || (!multi && n != 1)) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  std::vector<GraphCsr> g((size_t)n);
  std::vector<BnView> bn((size_t)n);
  for (int i = 0; i < n; ++i)
    if (desc[i].kind != desc[0].kind || !dbg_edge_ok(desc[i], g[(size_t)i], bn[(size_t)i])) return SLN_E_BADARG;
  if (variant) *variant = -1;
  if (!multi) return edge_single(desc[0], g[0], bn[0], st);
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  switch (desc[0].kind) {
    case E_SCATTER_FWD: {
      std::vector<MScatterFwd> rooms((size_t)n);
      for (int i = 0; i < n; ++i) { const SlnDbgEdge& d = desc[i]; rooms[(size_t)i] = MScatterFwd{d.a, d.lda, d.H, d.D, bn[(size_t)i], g[(size_t)i], d.rows, d.out, 0, 0}; }
      return edge_multi(rooms, [](MScatterFwd& m) { return sln_plan_scatter_avg_fwd(m); }, [](const MScatterFwd* t, int R, int var, int gx, int gy, hipStream_t s) { return sln_launch_scatter_avg_fwd_multi(t, R, var, gx, gy, s); }, variant, st);
    }
    case E_SCATTER_BWD: {
      std::vector<MScatterBwd> rooms((size_t)n);
      for (int i = 0; i < n; ++i) {
        const SlnDbgEdge& d = desc[i];
        rooms[(size_t)i] = MScatterBwd{d.a, d.b, d.ldb, d.col0, d.c, d.ldc, d.H, d.D, bn[(size_t)i], g[(size_t)i], d.rows, d.out, d.gsums, d.cstride, 0, 0};
      }
      return edge_multi(rooms, [](MScatterBwd& m) { return sln_plan_scatter_avg_bwd(m); }, [](const MScatterBwd* t, int R, int var, int gx, int gy, hipStream_t s) { return sln_launch_scatter_avg_bwd_multi(t, R, var, gx, gy, s); }, variant, st);
    }
    case E_GATHER_BWD: {
      std::vector<MGatherBwd> rooms((size_t)n);
      for (int i = 0; i < n; ++i) {
        const SlnDbgEdge& d = desc[i];
        rooms[(size_t)i] = MGatherBwd{d.a, d.lda, d.D, g[(size_t)i], d.rows, d.b, d.ldb, d.c, d.ldc, bn[(size_t)i], d.masked, d.out, d.ldo, d.gsums, d.cstride, 0, 0};
      }
      return edge_multi(rooms, [](MGatherBwd& m) { return sln_plan_gather_bwd(m); }, [](const MGatherBwd* t, int R, int var, int gx, int gy, hipStream_t s) { return sln_launch_gather_bwd_multi(t, R, var, gx, gy, s); }, variant, st);
    }
    case E_MASK_GSTATS: {
      std::vector<MMaskGstats> rooms((size_t)n);
      for (int i = 0; i < n; ++i) {
        const SlnDbgEdge& d = desc[i];
        rooms[(size_t)i] = MMaskGstats{d.a, d.lda, d.b, d.ldb, d.c, d.ldc, bn[(size_t)i], d.rows, d.cols, d.out, d.ldo, d.gsums, d.cstride, 0, 0};
      }
      return edge_multi(rooms, [](MMaskGstats& m) { return sln_plan_mask_gstats(m); }, [](const MMaskGstats* t, int R, int, int gx, int gy, hipStream_t s) { return sln_launch_mask_gstats_multi(t, R, gx, gy, s); }, variant, st);
    }
    case E_ADD2: {
      std::vector<MAdd2> rooms((size_t)n);
      for (int i = 0; i < n; ++i) { const SlnDbgEdge& d = desc[i]; rooms[(size_t)i] = MAdd2{d.a, d.lda, d.b, d.ldb, d.rows, d.cols, d.out, d.ldo, 0, 0}; }
      return edge_multi(rooms, [](MAdd2& m) { return sln_plan_add2(m); }, [](const MAdd2* t, int R, int, int gx, int, hipStream_t s) { return sln_launch_add2_multi(t, R, gx, s); }, variant, st);
    }
  }
  return SLN_E_BADARG;                       // bn_relu_apply has no multi form
}

extern "C" int sln_debug_vae_embed(const SlnDbgEmbed* desc, int n, int multi, int* variant, void* stream) {
  if (!desc || n < 1 || n > 64 || (!multi && n != 1)) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n; ++i)
    if (desc[i].kind != desc[0].kind || !dbg_embed_ok(desc[i])) return SLN_E_BADARG;
  if (variant) *variant = -1;
  if (!multi) return embed_single(desc[0], st);
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  switch (desc[0].kind) {
    case M_DEC: {
      std::vector<MDecAssemble> rooms((size_t)n);
      for (int i = 0; i < n; ++i) rooms[(size_t)i] = MDecAssemble{dbg_dec(desc[i]), 0, 0};
      return edge_multi(rooms, [](MDecAssemble& m) { return sln_plan_dec_assemble(m); },
                        [](const MDecAssemble* t, int R, int, int gx, int, hipStream_t s) { return sln_launch_dec_assemble_multi(t, R, gx, s); }, variant, st);
    }
    case M_DEC_BWD: return dec_bwd_multi(desc, n, variant, st);
    case M_GATHER: {
      std::vector<MEmbedGather> rooms((size_t)n);
      for (int i = 0; i < n; ++i) { const SlnDbgEmbed& d = desc[i]; rooms[(size_t)i] = MEmbedGather{static_cast<const int*>(d.idx), d.src, d.O, d.n, static_cast<float*>(d.dst), 0, 0}; }
      return edge_multi(rooms, [](MEmbedGather& m) { return sln_plan_embed_gather(m); },
                        [](const MEmbedGather* t, int R, int, int gx, int, hipStream_t s) { return sln_launch_embed_gather_multi(t, R, gx, s); }, variant, st);
    }
    case M_BWD_I32: case M_BWD_I64: {
      const int i64 = desc[0].kind == M_BWD_I64;
      std::vector<MEmbedBwd> rooms((size_t)n);
      int smem = 0;
      for (int i = 0; i < n; ++i) {
        const SlnDbgEmbed& d = desc[i];
        rooms[(size_t)i] = MEmbedBwd{d.idx, d.src, d.ld, d.col0, d.O, d.n, d.table_rows, 0, static_cast<float*>(d.dst), 0, 0};
        smem = d.table_rows * d.n > smem ? d.table_rows * d.n : smem;
      }
      return edge_multi(rooms, [i64](MEmbedBwd& m) { return sln_plan_embed_bwd(m, i64); },
                        [smem](const MEmbedBwd* t, int R, int var, int gx, int gy, hipStream_t s) {
                          return sln_launch_embed_bwd_multi(t, R, var, gx, gy, (var & 3) == MV_EMBED_LDS ? smem : 0, s);
                        }, variant, st);
    }
  }
  return SLN_E_BADARG;                       // the other kinds have no multi form
}

extern "C" int sln_debug_vae_loss(const SlnDbgLoss* d, void* stream) {
  if (!d || d->O < 1) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  switch (d->kind) {
    case 0: {
      if (!d->boxes || !d->boxes_pred || !d->angles || !d->angles_pred || !d->acc || !d->losses || d->box_dim < 1 || d->n_angle < 1) return SLN_E_BADARG;
      if (d->from_logits && !d->logits) return SLN_E_BADARG;
      if (!d->use_ae && (!d->mu || !d->logvar || !d->kl_weight || d->n_z < 1)) return SLN_E_BADARG;
      if (d->d_boxes_pred && d->ld_dbp < d->box_dim) return SLN_E_BADARG;
      LossArgs a; std::memset(&a, 0, sizeof(a));
      a.boxes = d->boxes; a.boxes_pred = d->boxes_pred; a.box_dim = d->box_dim; a.angles = d->angles; a.logits = d->logits;
      a.angles_pred = d->angles_pred; a.n_angle = d->n_angle; a.mu = d->mu; a.logvar = d->logvar; a.n_z = d->n_z; a.use_ae = d->use_ae;
      a.kl_weight = d->kl_weight; a.O = d->O; a.acc = d->acc; a.losses = d->losses; a.d_boxes_pred = d->d_boxes_pred; a.d_logits = d->d_logits;
      a.ld_dbp = d->ld_dbp; a.acc_prezeroed = d->acc_prezeroed; a.from_logits = d->from_logits;
      return sln_launch_loss(a, st);
    }
    case 1:
      if (!d->logits || !d->angles_pred || d->n_angle < 1) return SLN_E_BADARG;
      return sln_launch_log_softmax(d->logits, d->angles_pred, d->O, d->n_angle, st);
    case 2:
      if (!d->angles_pred || !d->d_logprob || !d->d_logits || d->n_angle < 1) return SLN_E_BADARG;
      return sln_launch_log_softmax_bwd(d->angles_pred, d->d_logprob, d->d_logits, d->O, d->n_angle, st);
    case 3:
      if (!d->dz || !d->dmu || !d->dlogvar || d->n_z < 1) return SLN_E_BADARG;
      if (!d->use_ae && (!d->mu || !d->logvar || !d->eps || !d->kl_weight)) return SLN_E_BADARG;
      return sln_launch_latent_bwd(d->mu, d->logvar, d->eps, d->dz, d->kl_weight, d->O, d->n_z, d->use_ae, d->dmu, d->dlogvar, st);
  }
  return SLN_E_BADARG;
}

extern "C" int sln_debug_vae_tables(int kind, const void* entries_host, int n, int width, float momentum, int independent, int rows_t,
                                    int rows_o, void* stream) {
  if (!entries_host || n < 1 || n > 4096 || width < 1 || kind < 0 || kind > 2) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  if (kind == 2) {
    const SlnDbgTranspose* e = static_cast<const SlnDbgTranspose*>(entries_host);
    std::vector<TransposeEntry> h((size_t)n);
    for (int i = 0; i < n; ++i) {
      if (!e[i].src || !e[i].dst || e[i].rows < 1 || e[i].cols < 1 || e[i].dst_ld < e[i].rows) return SLN_E_BADARG;
      if (((e[i].rows + 31) / 32) * ((e[i].cols + 31) / 32) > width) return SLN_E_BADARG;          // max_tiles must cover every entry
      h[(size_t)i] = TransposeEntry{e[i].src, e[i].dst, e[i].rows, e[i].cols, e[i].dst_ld, 0};
    }
    DevTable<TransposeEntry> tab;
    int r = tab.upload(h);
    if (!r) r = sln_launch_transpose_table(tab.p, n, width, st);
    return tab.finish(r, st);
  }
  const SlnDbgBnEntry* e = static_cast<const SlnDbgBnEntry*>(entries_host);
  std::vector<BnTableEntry> h((size_t)n);
  for (int i = 0; i < n; ++i) {
    const SlnDbgBnEntry& s = e[i];
    if (s.C < 1 || s.C > width || s.cstride < s.C) return SLN_E_BADARG;
    if (kind == 0) {
      const int rows = s.rows == -1 ? rows_t : (s.rows == -2 ? rows_o : s.rows);
      if (rows < 1 || (s.rmean && (!s.sums || !s.rvar))) return SLN_E_BADARG;
    } else if (s.dgamma && (!s.gsums || !s.dbeta)) return SLN_E_BADARG;
    BnTableEntry& t = h[(size_t)i];
    std::memset(&t, 0, sizeof(t));
    t.sums = s.sums; t.gsums = s.gsums; t.cstride = s.cstride; t.C = s.C; t.rows = s.rows;
    t.rmean = s.rmean; t.rvar = s.rvar; t.nbt = s.nbt; t.dgamma = s.dgamma; t.dbeta = s.dbeta;
  }
  DevTable<BnTableEntry> tab;
  int r = tab.upload(h);
  if (!r) r = kind == 0 ? sln_launch_bn_running_update(tab.p, n, width, momentum, independent, st, rows_t, rows_o)
                        : sln_launch_bn_param_grads(tab.p, n, width, independent, st);
  return tab.finish(r, st);
}

extern "C" int sln_debug_vae_opt(SlnDbgOpt* d, void* stream) {
  if (!d || d->calls < 1 || d->calls > 8 || d->kind < 0 || d->kind > 2) return SLN_E_BADARG;
  if (d->kind == 0 && (!d->grads || !d->m || !d->v || d->step < 0)) return SLN_E_BADARG;
  if (d->kind == 2 ? (d->params && d->n < 1) : (!d->params || d->n < 1)) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  StepPrologue pro; std::memset(&pro, 0, sizeof(pro));
  if (d->kind == 2) {
    const SlnDbgEmbed* e = d->pro;
    if (!e || !dbg_enc(*e, pro.enc) || e->T < 0 || e->zero_bytes < 0 || e->zero_bytes % 16 || (reinterpret_cast<uintptr_t>(e->zero_ptr) & 15)) return SLN_E_BADARG;
    if (e->T > 0 && (!e->idx || !e->src || !e->dst || e->n < 1 || !e->src2 || !e->dst2 || e->n2 < 1)) return SLN_E_BADARG;
    pro.eps = d->params; pro.n_eps = (long)d->n;
    pro.pidx = static_cast<const int*>(e->idx); pro.T = e->T;
    pro.pemb_ec = e->src; pro.n_ec = e->n; pro.p0e = static_cast<float*>(e->dst);
    pro.pemb_dc = e->src2; pro.n_dc = e->n2; pro.p0d = static_cast<float*>(e->dst2);
    pro.zero_ptr = e->zero_ptr; pro.zero_bytes = (long)e->zero_bytes;
  }
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  std::vector<AdamScalars> h(1);
  std::memset(h.data(), 0, sizeof(AdamScalars));
  h[0].step = d->step; h[0].lr = d->lr; h[0].beta1 = d->beta1; h[0].beta2 = d->beta2; h[0].eps = d->eps;
  h[0].rng_seed = d->seed; h[0].rng_offset = d->offset;
  DevTable<AdamScalars> sc;
  int r = sc.upload(h);
  pro.scalars = sc.p;
  for (int k = 0; k < d->calls && !r; ++k)
    r = d->kind == 0   ? sln_launch_adam(d->params, d->grads, d->m, d->v, (long)d->n, sc.p, d->total_loss, st)
        : d->kind == 1 ? sln_launch_randn(d->params, (long)d->n, sc.p, st)
                       : sln_launch_step_prologue(pro, st);
  const int rs = (int)hipStreamSynchronize(st);
  if (!r) r = rs;
  if (!r) r = (int)hipMemcpy(h.data(), sc.p, sizeof(AdamScalars), hipMemcpyDeviceToHost);
  if (sc.p) (void)hipFree(sc.p);
  if (r) return r;
  d->out_step = h[0].step; d->out_offset = h[0].rng_offset; d->out_bc1 = h[0].bc1; d->out_bc2 = h[0].bc2; d->out_skip = h[0].skip;
  if (h[0].adam_done != 0 || h[0].rng_done != 0) return SLN_E_STATE;        // an arrival ticket that did not reset
  return 0;
}

extern "C" int64_t sln_debug_vae_leaf_launches(const SlnVae* h) { return h ? (int64_t)sln_vae_engine_leaf_launches(h) : (int64_t)SLN_E_BADARG; }
extern "C" int64_t sln_debug_vae_tail_launches(const SlnVae* h) { return h ? (int64_t)sln_vae_engine_tail_launches(h) : (int64_t)SLN_E_BADARG; }
extern "C" int64_t sln_debug_vae_half_launches(const SlnVae* h) { return h ? (int64_t)sln_vae_engine_half_launches(h) : (int64_t)SLN_E_BADARG; }
extern "C" int64_t sln_debug_vae_graph_captures(const SlnVae* h) { return h ? (int64_t)sln_vae_engine_graph_captures(h) : (int64_t)SLN_E_BADARG; }
