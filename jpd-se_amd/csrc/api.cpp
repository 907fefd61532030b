// Library-level entry points: version, error string, architecture check.
#include "common.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace jpdse {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(JPDSE_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return JPDSE_OK;
}

// jpdse_code_import (binarize.hip): everything that can be refused without a device
int code_import_check(int dtype, int N, int H, int W, int C, const void* in, const void* b) {
  JPDSE_REQUIRE(!bad_dtype(dtype), "code_import: bad dtype %d", dtype);
  JPDSE_REQUIRE(in != nullptr && b != nullptr, "code_import: null pointer");
  JPDSE_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "code_import: non-positive extent (N %d, H %d, W %d, C %d)", N, H, W, C);
  return JPDSE_OK;
}

// jpdse_vq_* (vq.hip, vq_bottleneck.hip): everything that can be refused without a device
int vq_shape_check(const char* who, int M, int D, int L) {
  JPDSE_REQUIRE(D >= 1 && D <= 32, "%s: center_size D = %d (1 .. 32)", who, D);
  JPDSE_REQUIRE(L >= 2 && L <= 512, "%s: n_center L = %d (2 .. 512)", who, L);
  JPDSE_REQUIRE(M >= 1, "%s: M = %d vectors (at least 1)", who, M);
  JPDSE_REQUIRE((long long)M * L < (1LL << 31), "%s: M * L = %lld (below 2^31)", who, (long long)M * L);
  return JPDSE_OK;
}

static int vq_sigma_check(const char* who, float sigma) {
  JPDSE_REQUIRE(isfinite(sigma) && sigma > 0.f, "%s: sigma is %g (a finite value > 0)", who, (double)sigma);
  return JPDSE_OK;
}

int vq_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  JPDSE_REQUIRE(ws != nullptr && ws_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", who,
                ws ? ws_bytes : (size_t)0, need);
  return JPDSE_OK;
}

int vqb_common_check(const char* who, int dtype, int M, int D, int L, float sigma) {
  JPDSE_REQUIRE(!bad_dtype(dtype), "%s: bad dtype %d", who, dtype);
  if (int rc = vq_shape_check(who, M, D, L)) return rc;
  return vq_sigma_check(who, sigma);
}

// jpdse_vq_res_* (vq_residual.hip): S books, of which the first n are in use
// lowest: 0 for the calls that admit a quantizer without a stage in use, 1 for every other
int vq_res_check(const char* who, int dtype, int M, int D, int L, int S, int n, int lowest) {
  JPDSE_REQUIRE(!bad_dtype(dtype), "%s: bad dtype %d", who, dtype);
  if (int rc = vq_shape_check(who, M, D, L)) return rc;
  JPDSE_REQUIRE(S >= 1 && S <= JPDSE_VQ_RES_MAX_STAGES, "%s: S = %d stages (1 .. %d)", who, S, JPDSE_VQ_RES_MAX_STAGES);
  JPDSE_REQUIRE(n >= 0 && n <= S, "%s: n_stages = %d (0 .. S = %d)", who, n, S);
  JPDSE_REQUIRE(n >= lowest, "%s: n_stages = %d (%d .. S = %d)", who, n, lowest, S);
  return JPDSE_OK;
}

int vqr_group_check(const char* who, int M, int L, int G) {
  JPDSE_REQUIRE(G >= 1, "%s: G = %d groups (at least 1)", who, G);
  JPDSE_REQUIRE(M % G == 0, "%s: G = %d does not divide M = %d", who, G, M);
  JPDSE_REQUIRE((long long)G * L <= 65536, "%s: G * L = %lld (at most 65536)", who, (long long)G * L);
  return JPDSE_OK;
}

// the grouped jpdse_vq_res_* calls (vq_res_ec.hip, vq_res_rate.hip, jpdse_vq_res_bwd_grouped): at least one
// stage in use, the groups, and tables [n][G][L] of at most kVqResCells cells
int vq_res_grouped_check(const char* who, int dtype, int M, int D, int L, int S, int n, int G) {
  if (int rc = vq_res_check(who, dtype, M, D, L, S, n, 1)) return rc;
  if (int rc = vqr_group_check(who, M, L, G)) return rc;
  JPDSE_REQUIRE((long long)n * G * L <= kVqResCells, "%s: n_stages * G * L = %lld (at most %d)", who, (long long)n * G * L, kVqResCells);
  return JPDSE_OK;
}

int vq_soft_fwd_check(const jpdse_vq_soft_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_soft_fwd: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_soft_fwd: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_soft_fwd", a->M, a->D, a->L)) return rc;
  if (int rc = vq_sigma_check("vq_soft_fwd", a->sigma)) return rc;
  JPDSE_REQUIRE(a->x && a->code_book && a->p, "vq_soft_fwd: null pointer");
  return JPDSE_OK;
}

int vq_hard_fwd_check(const jpdse_vq_hard_fwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_hard_fwd: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_hard_fwd: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_hard_fwd", a->M, a->D, a->L)) return rc;
  JPDSE_REQUIRE(a->x && a->code_book && a->index, "vq_hard_fwd: null pointer");
  return JPDSE_OK;
}

int vq_soft_bwd_check(const jpdse_vq_soft_bwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_soft_bwd: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_soft_bwd: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_soft_bwd", a->M, a->D, a->L)) return rc;
  if (int rc = vq_sigma_check("vq_soft_bwd", a->sigma)) return rc;
  JPDSE_REQUIRE(a->dp && a->p && a->x && a->code_book, "vq_soft_bwd: null pointer");
  if (a->dcode_book != nullptr)
    if (int rc = vq_ws_check("vq_soft_bwd", a->ws, a->ws_bytes, vq_workspace_bytes(a->M, a->D, a->L))) return rc;
  return JPDSE_OK;
}

int vq_decode_check(const jpdse_vq_decode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_decode: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_decode: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_decode", a->M, a->D, a->L)) return rc;
  JPDSE_REQUIRE(a->index && a->code_book && a->y && a->status, "vq_decode: null pointer");
  return JPDSE_OK;
}

int vq_decode_bwd_check(const jpdse_vq_decode_bwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_decode_bwd: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_decode_bwd: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_decode_bwd", a->M, a->D, a->L)) return rc;
  JPDSE_REQUIRE(a->index && a->dy && a->dcode_book && a->status, "vq_decode_bwd: null pointer");
  return vq_ws_check("vq_decode_bwd", a->ws, a->ws_bytes, vq_workspace_bytes(a->M, a->D, a->L));
}

int vq_argmax_check(const jpdse_vq_argmax_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_argmax: null argument struct");
  if (int rc = vq_shape_check("vq_argmax", a->M, 1, a->L)) return rc;
  JPDSE_REQUIRE(a->s && a->index, "vq_argmax: null pointer");
  return JPDSE_OK;
}

int vq_pmf_check(const jpdse_vq_pmf_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_pmf: null argument struct");
  if (int rc = vq_shape_check("vq_pmf", a->M, 1, a->L)) return rc;
  JPDSE_REQUIRE(a->s && a->pmf, "vq_pmf: null pointer");
  return vq_ws_check("vq_pmf", a->ws, a->ws_bytes, vq_workspace_bytes(a->M, 1, a->L));
}

int vq_pmf_bwd_check(const jpdse_vq_pmf_bwd_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_pmf_bwd: null argument struct");
  if (int rc = vq_shape_check("vq_pmf_bwd", a->M, 1, a->L)) return rc;
  JPDSE_REQUIRE(a->dpmf && a->ds, "vq_pmf_bwd: null pointer");
  return JPDSE_OK;
}

// jpdse_vq_lloyd_* (vq_fit.hip)
int vq_lloyd_accum_check(const jpdse_vq_lloyd_accum_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_lloyd_accum: null argument struct");
  JPDSE_REQUIRE(!bad_dtype(a->dtype), "vq_lloyd_accum: bad dtype %d", a->dtype);
  if (int rc = vq_shape_check("vq_lloyd_accum", a->M, a->D, a->L)) return rc;
  JPDSE_REQUIRE(a->x && a->code_book && a->counts && a->sums && a->sse && a->far_dist && a->far_vec, "vq_lloyd_accum: null pointer");
  return vq_ws_check("vq_lloyd_accum", a->ws, a->ws_bytes, vq_lloyd_workspace_bytes(a->M, a->D, a->L));
}

int vq_lloyd_update_check(const jpdse_vq_lloyd_update_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_lloyd_update: null argument struct");
  if (int rc = vq_shape_check("vq_lloyd_update", 1, a->D, a->L)) return rc;
  JPDSE_REQUIRE(a->code_book && a->counts && a->sums && a->sse && a->far_dist && a->far_vec && a->report,
                "vq_lloyd_update: null pointer");
  return JPDSE_OK;
}

// jpdse_vq_index_* (vq_coder.hip): the limits, the closed forms of the sizes, and everything that can be
// refused without a device.  nb = max(1, bit_length(L - 1)) decisions per symbol; stream s of the S holds ceil((M - s) / S)
// symbols and its slot nb of them + 8 bytes, so the slots add up to nb M + 8 S and the capacity is that + the 4 S of the table.
int vq_index_bits(int L) {
  int nb = 1;
  while ((1 << nb) < L) ++nb;
  return nb;
}

static bool vq_index_in_limits(int M, int L, int S) {
  if (L < 2 || L > 512 || M < 1 || S < 1 || S > 65535 || S > M) return false;
  const long long nb = vq_index_bits(L);
  return nb * M < (1LL << 31) && nb * M + 12LL * S < (1LL << 31);
}

long long vq_index_capacity_bytes(int M, int L, int S) {
  return vq_index_in_limits(M, L, S) ? (long long)vq_index_bits(L) * M + 12LL * S : 0;
}

size_t vq_index_workspace_bytes(int M, int L, int S) {
  if (!vq_index_in_limits(M, L, S)) return 0;
  // the slots, then the lengths and the flags of the streams
  return align_up((size_t)vq_index_bits(L) * M + 8 * (size_t)S, 16) + 2 * (size_t)S * sizeof(int32_t);
}

static int vq_index_shape_check(const char* who, int M, int L, int S) {
  JPDSE_REQUIRE(L >= 2 && L <= 512, "%s: n_center L = %d (2 .. 512)", who, L);
  JPDSE_REQUIRE(M >= 1, "%s: M = %d indices (at least 1)", who, M);
  JPDSE_REQUIRE(S >= 1 && S <= 65535 && S <= M, "%s: S = %d streams (1 .. min(M, 65535), M = %d)", who, S, M);
  JPDSE_REQUIRE(vq_index_in_limits(M, L, S), "%s: M * nb = %lld or the capacity %lld (both below 2^31)", who,
                (long long)vq_index_bits(L) * M, (long long)vq_index_bits(L) * M + 12LL * S);
  return JPDSE_OK;
}

int vq_index_encode_check(const jpdse_vq_index_encode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_index_encode: null argument struct");
  if (int rc = vq_index_shape_check("vq_index_encode", a->M, a->L, a->S)) return rc;
  JPDSE_REQUIRE(a->index && a->out && a->size && a->status, "vq_index_encode: null pointer");
  const long long cap = vq_index_capacity_bytes(a->M, a->L, a->S);
  JPDSE_REQUIRE(a->out_bytes >= cap, "vq_index_encode: output of %lld bytes below the payload capacity %lld",
                (long long)a->out_bytes, cap);
  return vq_ws_check("vq_index_encode", a->ws, a->ws_bytes, vq_index_workspace_bytes(a->M, a->L, a->S));
}

int vq_index_decode_check(const jpdse_vq_index_decode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_index_decode: null argument struct");
  if (int rc = vq_index_shape_check("vq_index_decode", a->M, a->L, a->S)) return rc;
  JPDSE_REQUIRE(a->in && a->index && a->status, "vq_index_decode: null pointer");
  JPDSE_REQUIRE(a->in_bytes >= 4LL * a->S && a->in_bytes < (1LL << 31),
                "vq_index_decode: payload of %lld bytes, outside [%d (its length table), 2^31)", (long long)a->in_bytes, 4 * a->S);
  return JPDSE_OK;
}

// jpdse_vq_plane_* (vq_plane.hip): the same for the index planes.  K = ceil(h / strip_rows) strips, S = K G
// streams, M = h w G symbols of at most nb + 2 decisions each: the slots add up to (nb + 2) M + 8 S and the capacity is that +
// the 4 S of the table.
int vq_plane_streams(int h, int G, int strip_rows) { return (h + strip_rows - 1) / strip_rows * G; }

static bool vq_plane_in_limits(int h, int w, int G, int L, int strip_rows) {
  if (L < 2 || L > 512 || h < 1 || w < 1 || G < 1 || strip_rows < 1) return false;
  const long long hw = (long long)h * w;
  if (hw >= (1LL << 31) || hw * G >= (1LL << 31)) return false;
  const long long S = ((long long)h + strip_rows - 1) / strip_rows * G;
  return S <= 65535 && (vq_index_bits(L) + 2) * hw * G + 12 * S < (1LL << 31);
}

long long vq_plane_capacity_bytes(int h, int w, int G, int L, int strip_rows) {
  if (!vq_plane_in_limits(h, w, G, L, strip_rows)) return 0;
  return (long long)(vq_index_bits(L) + 2) * h * w * G + 12LL * vq_plane_streams(h, G, strip_rows);
}

size_t vq_plane_workspace_bytes(int h, int w, int G, int L, int strip_rows) {
  if (!vq_plane_in_limits(h, w, G, L, strip_rows)) return 0;
  // the slots, then the lengths and the flags of the streams
  const size_t S = (size_t)vq_plane_streams(h, G, strip_rows);
  return align_up((size_t)(vq_index_bits(L) + 2) * h * w * G + 8 * S, 16) + 2 * S * sizeof(int32_t);
}

static int vq_plane_shape_check(const char* who, int h, int w, int G, int L, int strip_rows) {
  JPDSE_REQUIRE(L >= 2 && L <= 512, "%s: n_center L = %d (2 .. 512)", who, L);
  JPDSE_REQUIRE(h >= 1 && w >= 1 && G >= 1, "%s: a plane of h = %d x w = %d cells in G = %d groups (each at least 1)", who, h, w, G);
  JPDSE_REQUIRE(strip_rows >= 1, "%s: strip_rows = %d (at least 1)", who, strip_rows);
  const long long S = ((long long)h + strip_rows - 1) / strip_rows * G;
  JPDSE_REQUIRE(S <= 65535, "%s: S = %lld streams (ceil(h / strip_rows) * G, at most 65535)", who, S);
  JPDSE_REQUIRE(vq_plane_in_limits(h, w, G, L, strip_rows), "%s: h * w * G = %lld indices or the capacity (both below 2^31)", who,
                (long long)h * w * G);
  return JPDSE_OK;
}

int vq_plane_encode_check(const jpdse_vq_plane_encode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_plane_encode: null argument struct");
  if (int rc = vq_plane_shape_check("vq_plane_encode", a->h, a->w, a->G, a->L, a->strip_rows)) return rc;
  JPDSE_REQUIRE(a->index && a->out && a->size && a->status, "vq_plane_encode: null pointer");
  const long long cap = vq_plane_capacity_bytes(a->h, a->w, a->G, a->L, a->strip_rows);
  JPDSE_REQUIRE(a->out_bytes >= cap, "vq_plane_encode: output of %lld bytes below the payload capacity %lld",
                (long long)a->out_bytes, cap);
  return vq_ws_check("vq_plane_encode", a->ws, a->ws_bytes, vq_plane_workspace_bytes(a->h, a->w, a->G, a->L, a->strip_rows));
}

int vq_plane_decode_check(const jpdse_vq_plane_decode_args* a) {
  JPDSE_REQUIRE(a != nullptr, "vq_plane_decode: null argument struct");
  if (int rc = vq_plane_shape_check("vq_plane_decode", a->h, a->w, a->G, a->L, a->strip_rows)) return rc;
  JPDSE_REQUIRE(a->in && a->index && a->status, "vq_plane_decode: null pointer");
  const int table = 4 * vq_plane_streams(a->h, a->G, a->strip_rows);
  JPDSE_REQUIRE(a->in_bytes >= table && a->in_bytes < (1LL << 31),
                "vq_plane_decode: payload of %lld bytes, outside [%d (its length table), 2^31)", (long long)a->in_bytes, table);
  return JPDSE_OK;
}

// jpdse_code_cost (code_cost.hip): T[v] = round(-log2(v / 2048) * 2^16) for v in 1 .. 2047, T[0] = T[2048] = 0 (a probability
// never leaves [31, 2017]: neither end is ever looked up).  fp64 on the host; v / 2048 is exact.
const uint32_t* code_cost_table_host() {
  struct Table {
    uint32_t t[2049];
    Table() {
      t[0] = t[2048] = 0;
      for (int v = 1; v < 2048; ++v) t[v] = (uint32_t)llround(-log2((double)v / 2048.0) * 65536.0);
    }
  };
  static const Table table;
  return table.t;
}

// the label path of the code-length maps (code_cost.hip, vq_cost.hip): log2(s) when H = s h and W = s w with s a power of
// two, else -1; and everything of a label map that can be refused without a device
static int cost_scale_shift(int H, int W, int h, int w) {
  for (int sh = 0; sh < 31; ++sh) {
    const long long s = 1LL << sh;
    if (s * h == H && s * w == W) return sh;
    if (s * h > H) break;
  }
  return -1;
}

int cost_label_check(const char* who, const void* class_units, const void* class_pixels, int H, int W, int h, int w, int C,
                     int n_classes, int* shift) {
  JPDSE_REQUIRE(class_units != nullptr && class_pixels != nullptr, "%s: null pointer class_units or class_pixels with a label map",
                who);
  JPDSE_REQUIRE(H > 0 && W > 0, "%s: non-positive extent (H %d, W %d)", who, H, W);
  *shift = cost_scale_shift(H, W, h, w);
  JPDSE_REQUIRE(*shift >= 0, "%s: H %d x W %d is not the same power-of-two multiple of h %d x w %d", who, H, W, h, w);
  JPDSE_REQUIRE(n_classes >= 1 && n_classes <= kCostClassesMax, "%s: n_classes %d outside [1, %d]", who, n_classes, kCostClassesMax);
  JPDSE_REQUIRE((long long)H * W <= kCostMaxUnits / C, "%s: H * W * C above 2^40 (H %d, W %d, C %d)", who, H, W, C);
  return JPDSE_OK;
}

// jpdse_vq_*_cost (vq_cost.hip).  The workspace: the cost table (2049 uint32, rounded up to 256 bytes), then the
// per-symbol costs uint32 [M] (used when the caller does not want them)
size_t vq_cost_workspace_bytes(long long M) { return align_up(2049 * sizeof(uint32_t), 256) + (size_t)M * sizeof(uint32_t); }

static int vq_cost_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  if (ws == nullptr || ws_bytes < need)
    return set_error(JPDSE_EWORKSPACE, "%s: workspace too small (%zu bytes, %zu needed)", who, ws ? ws_bytes : (size_t)0, need);
  JPDSE_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace not 16-byte aligned", who);
  return JPDSE_OK;
}

int vq_index_cost_check(const jpdse_vq_index_cost_args* a, int* shift) {
  JPDSE_REQUIRE(a != nullptr, "vq_index_cost: null argument struct");
  if (int rc = vq_index_shape_check("vq_index_cost", a->M, a->L, a->S)) return rc;
  JPDSE_REQUIRE(a->G >= 1 && a->M % a->G == 0, "vq_index_cost: G = %d groups (at least 1, dividing M = %d)", a->G, a->M);
  JPDSE_REQUIRE(a->index && a->cell && a->group && a->stream_units && a->stream_decisions && a->status,
                "vq_index_cost: null pointer");
  *shift = 0;
  if (a->label != nullptr) {
    JPDSE_REQUIRE(a->h >= 1 && a->w >= 1 && (long long)a->h * a->w * a->G == a->M,
                  "vq_index_cost: a cell grid of h = %d x w = %d in G = %d groups does not hold M = %d indices", a->h, a->w, a->G, a->M);
    if (int rc = cost_label_check("vq_index_cost", a->class_units, a->class_pixels, a->H, a->W, a->h, a->w, a->G, a->n_classes, shift))
      return rc;
  }
  return vq_cost_ws_check("vq_index_cost", a->ws, a->ws_bytes, vq_cost_workspace_bytes(a->M));
}

int vq_plane_cost_check(const jpdse_vq_plane_cost_args* a, int* shift) {
  JPDSE_REQUIRE(a != nullptr, "vq_plane_cost: null argument struct");
  if (int rc = vq_plane_shape_check("vq_plane_cost", a->h, a->w, a->G, a->L, a->strip_rows)) return rc;
  JPDSE_REQUIRE(a->index && a->cell && a->group && a->stream_units && a->stream_decisions && a->status,
                "vq_plane_cost: null pointer");
  *shift = 0;
  if (a->label != nullptr)
    if (int rc = cost_label_check("vq_plane_cost", a->class_units, a->class_pixels, a->H, a->W, a->h, a->w, a->G, a->n_classes, shift))
      return rc;
  return vq_cost_ws_check("vq_plane_cost", a->ws, a->ws_bytes, vq_cost_workspace_bytes((long long)a->h * a->w * a->G));
}

// ---- in-library timer for the HBM-bound calls (bench.py "roofline_hbm"): hipEvent pairs around whole InstanceNorm /
// Adam calls, recorded on the stream the kernels run on; each region carries the call's ALGORITHMIC bytes.
struct HbmProf {
  bool on = false;
  int used = 0;
  int max_regions = 0;          // of the CURRENT selection: `ev` only ever grows, `bytes` / `cls` are sized to this
  std::vector<hipEvent_t> ev;   // 2 per region
  std::vector<double> bytes;
  std::vector<int> cls;
};
static HbmProf g_hbm;

int hbm_prof_begin(hipStream_t s) {
  if (!g_hbm.on || g_hbm.used >= g_hbm.max_regions || (size_t)(2 * g_hbm.used + 2) > g_hbm.ev.size()) return -1;
  (void)hipEventRecord(g_hbm.ev[2 * g_hbm.used], s);
  return g_hbm.used++;
}

void hbm_prof_end(int slot, int cls, double bytes, hipStream_t s) {
  if (slot < 0) return;
  (void)hipEventRecord(g_hbm.ev[2 * slot + 1], s);
  g_hbm.bytes[slot] = bytes;
  g_hbm.cls[slot] = cls;
}

}  // namespace jpdse

extern "C" {

int jpdse_prof_hbm_select(int32_t enable, int32_t max_regions) {
  using jpdse::g_hbm;
  g_hbm.on = false;
  g_hbm.used = 0;
  g_hbm.max_regions = 0;
  if (!enable) return JPDSE_OK;
  JPDSE_REQUIRE(max_regions > 0, "prof_hbm_select: max_regions must be positive");
  while (g_hbm.ev.size() < (size_t)2 * max_regions) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return jpdse::set_error(JPDSE_ELAUNCH, "prof_hbm_select: hipEventCreate failed");
    g_hbm.ev.push_back(e);
  }
  g_hbm.bytes.assign(max_regions, 0.0);
  g_hbm.cls.assign(max_regions, -1);
  g_hbm.max_regions = max_regions;
  g_hbm.on = true;
  return JPDSE_OK;
}

int jpdse_prof_hbm_collect(int32_t cls, double* total_ms, double* total_bytes, int64_t* regions) {
  using jpdse::g_hbm;
  JPDSE_REQUIRE(total_ms && total_bytes && regions && cls >= 0 && cls <= 2, "prof_hbm_collect: bad argument");
  double ms = 0.0, by = 0.0;
  int64_t n = 0;
  for (int i = 0; i < g_hbm.used; ++i) {
    if (g_hbm.cls[i] != cls) continue;
    if (hipEventSynchronize(g_hbm.ev[2 * i + 1]) != hipSuccess)
      return jpdse::set_error(JPDSE_ELAUNCH, "prof_hbm_collect: hipEventSynchronize failed");
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_hbm.ev[2 * i], g_hbm.ev[2 * i + 1]) != hipSuccess)
      return jpdse::set_error(JPDSE_ELAUNCH, "prof_hbm_collect: hipEventElapsedTime failed");
    ms += t;
    by += g_hbm.bytes[i];
    ++n;
  }
  *total_ms = ms;
  *total_bytes = by;
  *regions = n;
  return JPDSE_OK;
}

int jpdse_code_cost_table(uint32_t* out) {
  JPDSE_REQUIRE(out != nullptr, "code_cost_table: null pointer");
  memcpy(out, jpdse::code_cost_table_host(), 2049 * sizeof(uint32_t));
  return JPDSE_OK;
}

size_t jpdse_vq_index_cost_workspace_size(int32_t M, int32_t L, int32_t S, int32_t G, int32_t n_classes) {
  if (jpdse::vq_index_workspace_bytes(M, L, S) == 0 || G < 1 || M % G != 0 || n_classes < 0 || n_classes > jpdse::kCostClassesMax) return 0;
  return jpdse::vq_cost_workspace_bytes(M);
}

size_t jpdse_vq_plane_cost_workspace_size(int32_t h, int32_t w, int32_t G, int32_t L, int32_t strip_rows, int32_t n_classes) {
  if (jpdse::vq_plane_workspace_bytes(h, w, G, L, strip_rows) == 0 || n_classes < 0 || n_classes > jpdse::kCostClassesMax) return 0;
  return jpdse::vq_cost_workspace_bytes((long long)h * w * G);
}

int jpdse_version(void) { return JPDSE_ABI_VERSION; }

const char* jpdse_last_error(void) { return jpdse::g_err; }

int jpdse_arch_check(int device) {
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return jpdse::set_error(JPDSE_EARCH, "hipGetDeviceProperties(%d): %s", device, hipGetErrorString(e));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return jpdse::set_error(JPDSE_EARCH, "device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
  return JPDSE_OK;
}

}  // extern "C"
