// Beam-search step on the device (model/prismer_caption.py:45-50, model/prismer_vqa.py:52-58 run transformers' beam search: 3 beams).
//   ph_beam_topk     log-softmax + beam score + EOS ban + the best 2*nb (beam, token) candidates of every image, in a DEFINED order
//   ph_beam_topk_edit  the same with the repetition penalty and the n-gram ban applied to the log-probabilities of the history's tokens
//   ph_beam_advance  the bookkeeping of one step (BeamSearchScorer.process + BeamHypotheses.add / is_done of transformers 4.26.1), the
//                    device form of prismer_amd/model/generate.py::beam_search_from_logits
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "decode_edit.h"

namespace {

constexpr int BT_THREADS = 256;
constexpr int BT_NV = 4;                               // 16-byte vectors a thread keeps in registers
constexpr int BT_CHUNK_VEC = BT_THREADS * BT_NV;       // vectors (8 columns each) one block covers at most: 8192 columns
constexpr int BT_KMAX = 16;                            // 2 * nb, nb <= 8
constexpr int BT_REC = 2 + 2 * BT_KMAX;                // words of one partial record: max, sum of exponentials, K x (logit, token)
constexpr int BT_MAX_SPLIT = 64;                       // the merge kernel folds the partial (max, sum) pairs of a row with one wave

// blocks a logit row is split over: enough to hold the row in registers (8192 columns per block), more while the launch is small
// (rows = 3 .. 96 would fill only that many CUs), never chunks below 1024 columns
int beam_nsplit(int64_t rows, int64_t V) {
  const int64_t need = (V + 8 * BT_CHUNK_VEC - 1) / (8 * BT_CHUNK_VEC);
  int64_t want = (512 + rows - 1) / rows;
  if (want > 16) want = 16;
  const int64_t cap = (V + 1023) / 1024;
  if (want > cap) want = cap;
  return (int)(need > want ? need : want);
}

// order of the candidates of ONE row: logit descending, then column ascending (= score descending, flat index ascending: the score
// is a monotone function of the logit, and two equal logits of a row get bit-equal scores)
__device__ __forceinline__ bool col_before(float xa, int ia, float xb, int ib) { return xa > xb || (xa == xb && ia < ib); }

// Stage 1: block (split, row) reads its share of the row ONCE (16-byte vectors, kept in registers), leaves (max, sum exp(x - max)) and
// its K best (logit, column) pairs in the workspace record.  The K pairs come from K rounds of a block-wide arg-best over the
// threads' cached best candidates; only the thread that owned the winner looks through its registers again.
// EDIT (ph_beam_topk_edit): the columns of the row's history -- ids[row * hist_rep][0 : cur], every token the repetition penalty or
// the n-gram rule can touch -- are marked in an LDS bitmap of the block's own slice and stay out of the K best (they still count in
// max and sum); the merge kernel scores them one by one.  Work per block: cur tokens, nothing V-wide.
template <bool EDIT>
__global__ __launch_bounds__(BT_THREADS) void beam_topk_partial_kernel(const bf16* __restrict__ logits, int64_t ld, int V, int nsplit, int vec_per_split,
                                                                       int K, int eos_banned, float* __restrict__ ws, const int64_t* __restrict__ ids,
                                                                       int64_t ids_ld, int cur, int hist_rep) {
  __shared__ float shf[2][BT_THREADS / 64];
  __shared__ int shi[2][BT_THREADS / 64];
  __shared__ uint32_t hist_bits[EDIT ? BT_CHUNK_VEC * 8 / 32 : 1];
  const int row = blockIdx.y, split = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16* x = logits + (int64_t)row * ld;
  const int nvec = (V + 7) / 8;
  const int v0 = split * vec_per_split, v1 = min(v0 + vec_per_split, nvec);
  if constexpr (EDIT) {
    for (int i = tid; i < BT_CHUNK_VEC * 8 / 32; i += BT_THREADS) hist_bits[i] = 0;
    __syncthreads();
    const int64_t* h = ids + (int64_t)row * hist_rep * ids_ld;
    const int64_t c0 = (int64_t)v0 * 8, c1 = min((int64_t)v1 * 8, (int64_t)V);
    for (int t = tid; t < cur; t += BT_THREADS) {
      const int64_t tok = h[t];
      if (tok >= c0 && tok < c1) atomicOr(&hist_bits[(int)(tok - c0) >> 5], 1u << ((int)(tok - c0) & 31));
    }
    __syncthreads();
  }
  float v[BT_NV][8];
  uint32_t out_bits = 0;                               // EDIT: bit j * 8 + e = the thread's column (j, e) is a history token
  int col0[BT_NV];                                     // first column of the thread's j-th vector; V (= no valid column) when it has none
  float mx = -FLT_MAX;
#pragma unroll
  for (int j = 0; j < BT_NV; ++j) {
    const int c = v0 + j * BT_THREADS + tid;
    if (c < v1) {
      const bf16x8 tv = *reinterpret_cast<const bf16x8*>(x + (int64_t)c * 8);
      col0[j] = c * 8;
      if constexpr (EDIT) out_bits |= ((hist_bits[(c - v0) >> 2] >> (((c - v0) & 3) * 8)) & 0xFFu) << (j * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) { v[j][e] = (c * 8 + e < V) ? bf2f(tv[e]) : -INFINITY; mx = fmaxf(mx, v[j][e]); }
    } else {
      col0[j] = V;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] = -INFINITY;
    }
  }
  float se = 0.f;
#pragma unroll
  for (int j = 0; j < BT_NV; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) se += __expf(v[j][e] - mx);
  // block max / sum (fixed tree)
  float gm = wave_max(mx);
  if (lane == 0) shf[0][wave] = gm;
  __syncthreads();
  gm = fmaxf(fmaxf(shf[0][0], shf[0][1]), fmaxf(shf[0][2], shf[0][3]));
  float gs = wave_sum(se * __expf(mx - gm));
  if (lane == 0) shf[1][wave] = gs;
  __syncthreads();
  gs = (shf[1][0] + shf[1][1]) + (shf[1][2] + shf[1][3]);
  __syncthreads();
  float* rec = ws + ((int64_t)row * nsplit + split) * BT_REC;
  if (tid == 0) { rec[0] = gm; rec[1] = gs; }

  float lastx = INFINITY; int lasti = -1;              // the thread's last emitted candidate: everything at or before it is out
  float bx; int bi;
  auto scan = [&]() {
    bx = -INFINITY; bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < BT_NV; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = col0[j] + e;
        const float xv = v[j][e];
        if (EDIT && ((out_bits >> (j * 8 + e)) & 1u)) continue;
        if (col < V && col != eos_banned && col_before(lastx, lasti, xv, col) && col_before(xv, col, bx, bi)) { bx = xv; bi = col; }
      }
  };
  scan();
  for (int r = 0; r < K; ++r) {
    float wx = bx; int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ox = __shfl_xor(wx, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (col_before(ox, oi, wx, wi)) { wx = ox; wi = oi; }
    }
    if (lane == 0) { shf[r & 1][wave] = wx; shi[r & 1][wave] = wi; }
    __syncthreads();
    wx = shf[r & 1][0]; wi = shi[r & 1][0];
#pragma unroll
    for (int w = 1; w < BT_THREADS / 64; ++w) {
      const float ox = shf[r & 1][w];
      const int oi = shi[r & 1][w];
      if (col_before(ox, oi, wx, wi)) { wx = ox; wi = oi; }
    }
    if (tid == 0) { rec[2 + 2 * r] = wx; reinterpret_cast<int*>(rec)[3 + 2 * r] = (wi == INT_MAX) ? -1 : wi; }
    if (wi == bi && wi != INT_MAX) { lastx = wx; lasti = wi; scan(); }
  }
}

// order of the candidates of one IMAGE: score descending, beam ascending, then the row's own order (logit descending, token
// ascending).  Where fp32 rounding leaves two different logits of a row with one score (|score| >> |logit|), the higher logit goes first.
struct Cand { float s; int beam; float x; int tok; };
__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
  if (a.s != b.s) return a.s > b.s;
  if (a.beam != b.beam) return a.beam < b.beam;
  return col_before(a.x, a.tok, b.x, b.tok);
}

// Stage 2: one wave per image.  lse of each of its rows from the partial (max, sum) pairs, score = beam_score + (x - lse) for the
// nb_in * nsplit * K surviving candidates, and K rounds of a wave-wide arg-best over them.
// EDIT: the history tokens the partial kernel left out come back as explicit candidates.  Per row, every DISTINCT history token inside
// [0, V) that the n-gram rule does not ban (and that is not the banned EOS) and whose logit is finite enters with
// beam_score + edit(x - lse), edit(l) = l * theta if l < 0 else l / theta (RepetitionPenaltyLogitsProcessor on the log-probability),
// x gathered from the logit row: at most cur gathers per row.  They live in dynamic LDS, nb_in * cur x (token, logit, score).
struct BeamEdit {
  const bf16* logits; int64_t ld; int V;
  const int64_t* ids; int64_t ids_ld; int cur, hist_rep, ngram, eos_banned;
  float theta;
};
template <bool EDIT>
__global__ __launch_bounds__(64) void beam_topk_merge_kernel(const float* __restrict__ ws, const float* __restrict__ beam_scores, int nb_in, int nsplit, int K,
                                                             float* __restrict__ top_score, int* __restrict__ top_beam, int* __restrict__ top_tok, BeamEdit ed) {
  __shared__ float s_lse[8], s_bs[8];
  extern __shared__ int edit_lds[];                    // EDIT: h_tok[cur], h_ban[cur], c_tok[nb_in * cur], c_x[..], c_s[..]
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int r = 0; r < nb_in; ++r) {
    const float* rec = ws + (((int64_t)b * nb_in + r) * nsplit + lane) * BT_REC;
    const float m = lane < nsplit ? rec[0] : -FLT_MAX;
    const float s = lane < nsplit ? rec[1] : 0.f;
    const float M = wave_max(m);
    const float tot = wave_sum(s * __expf(m - M));
    if (lane == 0) { s_lse[r] = M + logf(tot); s_bs[r] = beam_scores[(int64_t)b * nb_in + r]; }
  }
  __syncthreads();
  const int n_hist = EDIT ? nb_in * ed.cur : 0;
  int* const h_tok = edit_lds;
  int* const h_ban = h_tok + (EDIT ? ed.cur : 0);
  int* const c_tok = h_ban + (EDIT ? ed.cur : 0);
  float* const c_x = reinterpret_cast<float*>(c_tok + n_hist);
  float* const c_s = c_x + n_hist;
  if constexpr (EDIT) {
    const int cur = ed.cur, ng = ed.ngram;
    for (int r = 0; r < nb_in; ++r) {
      const int64_t q = (int64_t)b * nb_in + r;
      const int64_t* h = ed.ids + q * ed.hist_rep * ed.ids_ld;
      // h_tok[t] = the token at t, -1 outside the vocabulary; h_ban[t] = the n-gram that ends at t starts like the row's last n - 1 tokens
      for (int t = lane; t < cur; t += 64) {
        const int64_t tok = h[t];
        h_tok[t] = (tok >= 0 && tok < ed.V) ? (int)tok : -1;
        int ban = 0;
        if (ng > 0 && ng <= cur && t >= ng - 1) {
          ban = 1;
          for (int j = 0; j < ng - 1; ++j)
            if (h[t - ng + 1 + j] != h[cur - ng + 1 + j]) { ban = 0; break; }
        }
        h_ban[t] = ban;
      }
      __syncthreads();
      for (int t = lane; t < cur; t += 64) {
        const int tok = h_tok[t];
        bool ok = tok >= 0 && tok != ed.eos_banned;
        for (int u = 0; ok && u < cur; ++u)
          if (h_tok[u] == tok && (u < t || h_ban[u])) ok = false;      // an earlier copy stands for the token; a banned copy bans it
        float x = 0.f, sc = 0.f;
        if (ok) {
          x = bf2f(ed.logits[q * ed.ld + tok]);
          ok = fabsf(x) <= FLT_MAX;                    // finite: -inf is no candidate, a NaN never is
          const float l = x - s_lse[r];
          {
#pragma clang fp contract(off)
            sc = s_bs[r] + penalised(l, ed.theta);
          }
        }
        c_tok[r * cur + t] = ok ? tok : -1;
        c_x[r * cur + t] = x;
        c_s[r * cur + t] = sc;
      }
      __syncthreads();
    }
  }
  const int per_row = nsplit * K, n = nb_in * per_row;
  const Cand none = {-INFINITY, INT_MAX, -INFINITY, INT_MAX};
  Cand last = {INFINITY, -1, INFINITY, -1}, best;
  auto scan = [&]() {
    best = none;
    for (int i = lane; i < n; i += 64) {
      const int r = i / per_row, rem = i - r * per_row, sp = rem / K, k = rem - sp * K;
      const float* rec = ws + (((int64_t)b * nb_in + r) * nsplit + sp) * BT_REC;
      Cand c;
      c.x = rec[2 + 2 * k];
      c.tok = reinterpret_cast<const int*>(rec)[3 + 2 * k];
      if (c.tok < 0) continue;
      c.beam = r;
      c.s = s_bs[r] + (c.x - s_lse[r]);
      if (cand_before(last, c) && cand_before(c, best)) best = c;
    }
    if constexpr (EDIT)
      for (int i = lane; i < n_hist; i += 64) {
        if (c_tok[i] < 0) continue;
        const Cand c = {c_s[i], i / ed.cur, c_x[i], c_tok[i]};
        if (cand_before(last, c) && cand_before(c, best)) best = c;
      }
  };
  scan();
  for (int r = 0; r < K; ++r) {
    Cand w = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      Cand ot;
      ot.s = __shfl_xor(w.s, o, 64); ot.beam = __shfl_xor(w.beam, o, 64); ot.x = __shfl_xor(w.x, o, 64); ot.tok = __shfl_xor(w.tok, o, 64);
      if (cand_before(ot, w)) w = ot;
    }
    const bool found = w.tok != INT_MAX;
    if (lane == 0) {
      top_score[(int64_t)b * K + r] = found ? w.s : -INFINITY;
      top_beam[(int64_t)b * K + r] = found ? w.beam : 0;
      top_tok[(int64_t)b * K + r] = found ? w.tok : 0;
    }
    if (found && w.beam == best.beam && w.tok == best.tok) { last = w; scan(); }
  }
}

// One step of the search state, one wave per batch item.  Lane 0 walks the 2*nb candidates exactly as beam_search_from_logits does
// and leaves its decisions in LDS; all lanes then copy the token rows.
__global__ __launch_bounds__(64) void beam_advance_kernel(ph_beam_advance_args a) {
  __shared__ float h_score[8], nx_score[8];
  __shared__ int act_slot[8], act_beam[8], nx_beam[8], nx_tok[8], s_nact;
  const int b = blockIdx.x, lane = threadIdx.x, nb = a.nb, K = 2 * a.nb, cur = a.cur;
  if (lane == 0) {
    for (int k = 0; k < nb; ++k) { h_score[k] = a.hyp_score[b * nb + k]; nx_beam[k] = 0; nx_tok[k] = a.pad_token_id; nx_score[k] = 0.f; }
    int nh = a.n_hyp[b], dn = a.done[b], n_next = 0, n_act = 0;
    if (!dn) {
      for (int r = 0; r < K && n_next < nb; ++r) {
        const float s = a.top_score[b * K + r];
        const int bm = min(max(a.top_beam[b * K + r], 0), a.nb_in - 1), tk = a.top_tok[b * K + r];
        if (tk == a.eos_token_id) {
          if (r >= nb) continue;                        // an EOS ranked below the first nb candidates is dropped
          const float score = s / a.len_div;            // BeamHypotheses.add: sum_logprobs / cur_len ** length_penalty
          int slot = nh;
          bool ok = true;
          if (nh >= nb) {                               // full: replace the worst if strictly better
            slot = 0;
            for (int k = 1; k < nb; ++k) if (h_score[k] < h_score[slot]) slot = k;
            ok = score > h_score[slot];
          }
          if (ok) {
            h_score[slot] = score;
            act_slot[n_act] = slot; act_beam[n_act] = bm; ++n_act;
            a.hyp_len[b * nb + slot] = cur + 1;
            if (nh < nb) ++nh;
          }
        } else {
          nx_beam[n_next] = bm; nx_tok[n_next] = tk; nx_score[n_next] = s; ++n_next;
        }
      }
      float worst = h_score[0];
      for (int k = 1; k < nb; ++k) worst = fminf(worst, h_score[k]);
      if (nh >= nb && worst >= a.top_score[b * K] / a.len_div) dn = 1;
      for (int k = 0; k < nb; ++k) a.hyp_score[b * nb + k] = h_score[k];
      a.n_hyp[b] = nh;
      a.done[b] = dn;
    }
    s_nact = n_act;
  }
  __syncthreads();
  const int Tmax = a.Tmax, Bb = a.B * nb;
  const int n_act = s_nact;
  for (int i = 0; i < n_act; ++i) {                     // in order: a later hypothesis may take the slot of an earlier one
    const int64_t* src = a.ids_in + (int64_t)(b * nb + act_beam[i]) * Tmax;
    int64_t* dst = a.hyp_tok + (int64_t)(b * nb + act_slot[i]) * Tmax;
    for (int t = lane; t < Tmax; t += 64) dst[t] = (t == cur) ? (int64_t)a.eos_token_id : src[t];
  }
  for (int k = 0; k < nb; ++k) {
    const int64_t* src = a.ids_in + (int64_t)(b * nb + nx_beam[k]) * Tmax;
    int64_t* dst = a.ids_out + (int64_t)(b * nb + k) * Tmax;
    for (int t = lane; t < Tmax; t += 64) dst[t] = (t == cur) ? (int64_t)nx_tok[k] : src[t];
  }
  if (lane < nb) a.beam_scores[b * nb + lane] = nx_score[lane];
  for (int i = lane; i < a.rows_rep * nb; i += 64) {
    const int l = i / nb, k = i - l * nb;
    a.rows_out[(int64_t)l * Bb + b * nb + k] = l * Bb + b * a.nb_in + nx_beam[k];
  }
}

}  // namespace

int64_t beam_topk_workspace_bytes(int64_t B, int64_t nb, int64_t V) {
  if (B <= 0 || nb < 1 || nb > 8 || V < 2 * nb + 1 || V > (int64_t)BT_MAX_SPLIT * 8 * BT_CHUNK_VEC || B * nb > INT_MAX / 64) return -1;
  const int64_t one = B * beam_nsplit(B, V), all = B * nb * beam_nsplit(B * nb, V);
  return (one > all ? one : all) * BT_REC * 4;
}

namespace {
// the shared checks and launches of ph_beam_topk (ed == nullptr: the plain kernels) and ph_beam_topk_edit
int beam_topk_launch(const ph_beam_topk_args* a, const BeamEdit* ed, hipStream_t stream) {
  PH_CHECK_ARG(a && a->logits && a->beam_scores && a->workspace && a->top_score && a->top_beam && a->top_tok, "ph_beam_topk: null pointer");
  PH_CHECK_ARG(a->nb >= 1 && a->nb <= 8, "ph_beam_topk: num_beams %d outside 1..8", a->nb);
  PH_CHECK_ARG(a->nb_in == 1 || a->nb_in == a->nb, "ph_beam_topk: nb_in %d must be 1 or num_beams %d", a->nb_in, a->nb);
  PH_CHECK_ARG(a->B > 0 && (int64_t)a->B * a->nb <= INT_MAX / 64, "ph_beam_topk: bad batch size %d", a->B);
  PH_CHECK_ARG(a->V >= 2 * a->nb + 1, "ph_beam_topk: vocabulary %d below 2 * num_beams + 1 = %d", a->V, 2 * a->nb + 1);
  PH_CHECK_ARG((int64_t)a->V <= (int64_t)BT_MAX_SPLIT * 8 * BT_CHUNK_VEC, "ph_beam_topk: vocabulary %d above %d", a->V, BT_MAX_SPLIT * 8 * BT_CHUNK_VEC);
  PH_CHECK_ARG(a->ld >= a->V && (a->ld % 8) == 0 && (((uintptr_t)a->logits) & 15) == 0,
               "ph_beam_topk: logit rows must be 16-byte aligned (ld %lld: a multiple of 8 elements, >= V)", (long long)a->ld);
  PH_CHECK_ARG(!a->ban_eos || (a->eos_token_id >= 0 && a->eos_token_id < a->V), "ph_beam_topk: eos_token_id %d outside the vocabulary", a->eos_token_id);
  const int rows = a->B * a->nb_in, nsplit = beam_nsplit(rows, a->V), K = 2 * a->nb;
  PH_CHECK_ARG(a->workspace_bytes >= (int64_t)rows * nsplit * BT_REC * 4 && (((uintptr_t)a->workspace) & 3) == 0,
               "ph_beam_topk: workspace of %lld bytes, %lld needed (ph_query_workspace(PH_WS_BEAM_TOPK))", (long long)a->workspace_bytes,
               (long long)rows * nsplit * BT_REC * 4);
  const int nvec = (a->V + 7) / 8, vps = ceil_div(nvec, nsplit);
  ProfScope prof__(PH_FAM_MISC, 0.0, 2.0 * rows * (double)a->V, stream, "beam_topk");
  const int eos_banned = a->ban_eos ? a->eos_token_id : -1;
  if (!ed) {
    hipLaunchKernelGGL(beam_topk_partial_kernel<false>, dim3(nsplit, rows), dim3(BT_THREADS), 0, stream, (const bf16*)a->logits, a->ld, a->V, nsplit, vps,
                       K, eos_banned, (float*)a->workspace, (const int64_t*)nullptr, (int64_t)0, 0, 0);
    hipLaunchKernelGGL(beam_topk_merge_kernel<false>, dim3(a->B), dim3(64), 0, stream, (const float*)a->workspace, a->beam_scores, a->nb_in, nsplit, K,
                       a->top_score, a->top_beam, a->top_tok, BeamEdit{});
  } else {
    BeamEdit e = *ed;
    e.logits = (const bf16*)a->logits; e.ld = a->ld; e.V = a->V; e.hist_rep = a->nb / a->nb_in; e.eos_banned = eos_banned;
    hipLaunchKernelGGL(beam_topk_partial_kernel<true>, dim3(nsplit, rows), dim3(BT_THREADS), 0, stream, e.logits, a->ld, a->V, nsplit, vps, K, eos_banned,
                       (float*)a->workspace, e.ids, e.ids_ld, e.cur, e.hist_rep);
    hipLaunchKernelGGL(beam_topk_merge_kernel<true>, dim3(a->B), dim3(64), (size_t)(2 + 3 * a->nb_in) * e.cur * 4, stream, (const float*)a->workspace,
                       a->beam_scores, a->nb_in, nsplit, K, a->top_score, a->top_beam, a->top_tok, e);
  }
  PH_LAUNCH_CHECK("beam_topk kernels");
  return PH_OK;
}
}  // namespace

extern "C" int ph_beam_topk(const ph_beam_topk_args* a, hipStream_t stream) { return beam_topk_launch(a, nullptr, stream); }

extern "C" int ph_beam_topk_edit(const ph_beam_topk_args* a, const int64_t* ids, int64_t ids_ld, int cur, float repetition_penalty, int no_repeat_ngram_size,
                                 hipStream_t stream) {
  PH_CHECK_ARG(ids, "ph_beam_topk_edit: null ids");
  PH_CHECK_ARG(cur >= 1 && cur <= PH_EDIT_MAX_CUR && ids_ld >= cur, "ph_beam_topk_edit: history length %d outside 1..%d (row stride %lld)", cur, PH_EDIT_MAX_CUR,
               (long long)ids_ld);
  PH_CHECK_ARG(repetition_penalty > 0.f && repetition_penalty < INFINITY, "ph_beam_topk_edit: repetition_penalty must be a positive finite number");
  PH_CHECK_ARG(no_repeat_ngram_size >= 0, "ph_beam_topk_edit: no_repeat_ngram_size %d below 0", no_repeat_ngram_size);
  BeamEdit e{};
  e.ids = ids; e.ids_ld = ids_ld; e.cur = cur; e.ngram = no_repeat_ngram_size; e.theta = repetition_penalty;
  return beam_topk_launch(a, &e, stream);
}

extern "C" int ph_beam_advance(const ph_beam_advance_args* a, hipStream_t stream) {
  PH_CHECK_ARG(a && a->top_score && a->top_beam && a->top_tok && a->ids_in && a->ids_out && a->beam_scores && a->hyp_score && a->hyp_tok &&
               a->hyp_len && a->n_hyp && a->done && a->rows_out, "ph_beam_advance: null pointer");
  PH_CHECK_ARG(a->ids_in != a->ids_out, "ph_beam_advance: ids_in and ids_out must be different buffers");
  PH_CHECK_ARG(a->nb >= 1 && a->nb <= 8, "ph_beam_advance: num_beams %d outside 1..8", a->nb);
  PH_CHECK_ARG(a->nb_in == 1 || a->nb_in == a->nb, "ph_beam_advance: nb_in %d must be 1 or num_beams %d", a->nb_in, a->nb);
  PH_CHECK_ARG(a->B > 0 && (int64_t)a->B * a->nb <= INT_MAX / 64 && a->rows_rep >= 1 && a->rows_rep <= 64, "ph_beam_advance: bad batch size %d / rows_rep %d",
               a->B, a->rows_rep);
  PH_CHECK_ARG(a->Tmax > 0 && a->cur > 0 && a->cur < a->Tmax, "ph_beam_advance: position %d outside 1..Tmax-1 (Tmax %d)", a->cur, a->Tmax);
  PH_CHECK_ARG(a->len_div > 0.f && a->len_div < INFINITY, "ph_beam_advance: len_div must be cur ** length_penalty, a positive finite number");
  ProfScope prof__(PH_FAM_MISC, 0.0, 16.0 * a->B * a->nb * (double)a->Tmax, stream, "beam_advance");
  hipLaunchKernelGGL(beam_advance_kernel, dim3(a->B), dim3(64), 0, stream, *a);
  PH_LAUNCH_CHECK("beam_advance_kernel");
  return PH_OK;
}
