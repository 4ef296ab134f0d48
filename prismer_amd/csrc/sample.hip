// Sampled decoding step on the device (transformers generate(do_sample=True): MinLengthLogitsProcessor, TemperatureLogitsWarper,
// TopKLogitsWarper, TopPLogitsWarper, multinomial, and the bookkeeping of _sample), the device form of
// prismer_amd/model/generate.py::sample_from_logits.
//   ph_sample_step   one launch per decode step: filters, draws and does the step's bookkeeping for every row
//   ph_sample_step_edit   the same on the row after the repetition penalty (rounded back to bf16) and the n-gram ban
//
// One 1024-thread block per row.  bf16 logits take at most 65536 distinct values, so a counting histogram over the 16-bit
// order-preserving key IS the sorted distribution: packed 16-bit counts (V <= 65535: no carry) in 128 KB of LDS, filled by integer LDS
// atomics only, so the histogram does not depend on arrival order.  Everything after it -- the top-k threshold, the class masses
// cnt[key] * exp(z(key) - m), the top-p threshold, the class of the draw -- is a walk over the histogram, 64 bins per thread, highest keys
// on thread 0, joined by fixed-order block scans.  A second sweep over the row (L2-resident by then) finds the j-th member of the
// chosen class in ascending token order.  No float atomics: the same inputs give the same outputs on every run.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "decode_edit.h"

namespace {

constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_WORDS = 32768;                        // 65536 bins, two 16-bit counts per word
constexpr int SP_PHYS = SP_WORDS + SP_WORDS / 32;      // one pad word per 32: a thread's 32 words start 33 words after its neighbour's
constexpr int SP_MAX_VEC = 8;                          // 16-byte vectors per thread in a sweep: 8 * 1024 * 8 = 65536 columns

// bf16 bits -> key with key(a) < key(b) <=> a < b as numbers; -0 takes the key of +0 (one class of equal logits).  Finite values only.
__device__ __forceinline__ uint32_t key_of(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
__device__ __forceinline__ float val_of(uint32_t key) {
  const uint32_t b = (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu);
  return __uint_as_float(b << 16);
}
__device__ __forceinline__ bool bits_finite(uint32_t b) { return (b & 0x7F80u) != 0x7F80u; }

struct Scratch {
  float f[SP_WAVES];
  int i[SP_WAVES];
};

// exclusive prefix over the 1024 threads in thread order, and the total: Hillis-Steele inside a wave, the wave totals added in wave
// order -- one fixed association per thread, the same on every run
__device__ __forceinline__ float block_scan_f(float v, Scratch& s, float& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                     // the scratch may still be read from the call before
  if (lane == 63) s.f[wave] = inc;
  __syncthreads();
  float base = 0.f, tot = 0.f;
#pragma unroll
  for (int w = 0; w < SP_WAVES; ++w) {
    if (w == wave) base = tot;
    tot += s.f[w];
  }
  total = tot;
  return base + (inc - v);
}
__device__ __forceinline__ int block_scan_i(int v, Scratch& s, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) s.i[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SP_WAVES; ++w) {
    if (w == wave) base = tot;
    tot += s.i[w];
  }
  total = tot;
  return base + (inc - v);
}
__device__ __forceinline__ int block_max_i(int v, Scratch& s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) s.i[wave] = v;
  __syncthreads();
  int m = s.i[0];
#pragma unroll
  for (int w = 1; w < SP_WAVES; ++w) m = max(m, s.i[w]);
  return m;
}

// walks the thread's 64 bins from the highest key down: fn(key, count) for every non-empty bin; fn returns false to stop
template <typename F>
__device__ __forceinline__ void walk_bins(const uint32_t* hist, int chunk, F fn) {
  const uint32_t* w = hist + chunk * 33;
  for (int i = 31; i >= 0; --i) {
    const uint32_t wv = w[i];
    if (wv == 0) continue;
    const int key = chunk * 64 + 2 * i;
    if ((wv >> 16) && !fn(key + 1, (int)(wv >> 16))) return;
    if ((wv & 0xFFFFu) && !fn(key, (int)(wv & 0xFFFFu))) return;
  }
}

// bf16 bits of a history token's logit after the repetition penalty: fp32 product / IEEE quotient, rounded to nearest even
__device__ __forceinline__ uint32_t edit_bits(uint32_t b, float theta) {
  return (uint32_t)__builtin_bit_cast(unsigned short, f2bf(penalised(__uint_as_float(b << 16), theta)));
}

constexpr int SP_BITS = 65536 / 32;                    // words of a one-bit-per-column map

// EDIT (ph_sample_step_edit): two more LDS maps, one bit per column -- `seen` (the column is a token of the row's history
// ids[r][0 : cur]) and `ban` (the n-gram rule bans it) -- filled from the <= 512 history tokens, one per thread, before sweep 1.  A seen
// column enters the histogram under the key of its penalised bf16 value, a banned one is left out like the banned EOS, and sweep 2 applies
// the same transform.  The raw row's log-sum-exp needs the RAW histogram: each distinct history token has one owner thread (the one
// whose atomicOr set the bit) that moves its count from the edited to the raw bin (banned tokens: adds it) with integer LDS atomics
// before the raw sum is walked and moves it back afterwards, so that sum is over exact counts, in the plain kernel's order.
template <bool EDIT>
__global__ __launch_bounds__(SP_THREADS) void sample_step_kernel(ph_sample_step_args a, float theta, int ngram) {
  __shared__ uint32_t hist[SP_PHYS];
  __shared__ uint32_t seen_bits[EDIT ? SP_BITS : 1], ban_bits[EDIT ? SP_BITS : 1];
  __shared__ Scratch sc;
  __shared__ int s_bad, s_kth, s_cnt_ge, s_kept_cnt, s_hit, s_hit_j, s_tok;
  __shared__ float s_eos_x, s_kept_mass, s_raw_x;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int V = a.V, cur = a.cur;
  const int64_t out_i = (int64_t)r * a.Tmax + cur;

  const u32x4 rnd = philox4x32((uint32_t)r, (uint32_t)cur, 0u, 0x5a3b1eu, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const float u = (float)(rnd[0] >> 8) * (1.0f / 16777216.0f);

  if (a.done[r]) {                                     // a finished row emits pad and stays finished (block-uniform branch)
    if (tid == 0) {
      a.ids[out_i] = a.pad_token_id;
      if (a.u_out) a.u_out[r] = u;
      if (a.thr_out) a.thr_out[r] = INFINITY;
      if (a.kept_count_out) a.kept_count_out[r] = 0;
      if (a.kept_mass_out) a.kept_mass_out[r] = 0.f;
    }
    return;
  }

  for (int i = tid; i < SP_PHYS; i += SP_THREADS) hist[i] = 0;
  if constexpr (EDIT)
    for (int i = tid; i < SP_BITS; i += SP_THREADS) { seen_bits[i] = 0; ban_bits[i] = 0; }
  if (tid == 0) { s_bad = 0; s_eos_x = -INFINITY; s_kth = 0; s_hit_j = 0; s_tok = a.eos_token_id; s_raw_x = 0.f; }
  __syncthreads();

  const bf16* x = reinterpret_cast<const bf16*>(a.logits) + (int64_t)(r / a.rows_per_logit) * a.ld;
  const int nvec = (V + 7) >> 3;                        // ld >= V and ld % 8 == 0: the last vector lies inside the row
  const int banned = a.ban_eos ? a.eos_token_id : -1;

  // ---- EDIT: the history maps; thread t < cur takes history token t (cur <= 512)
  int own_kr = -1, own_ke = -1;                        // the owner's raw key (the token's raw logit is finite) / edited key (it is in the histogram)
  if constexpr (EDIT) {
    const int64_t* h = a.ids + (int64_t)r * a.Tmax;
    int e_tok = -1;
    bool own = false;
    if (tid < cur) {
      const int64_t tok = h[tid];
      if (tok >= 0 && tok < V) {                        // a token outside the vocabulary is never an index
        e_tok = (int)tok;
        own = !((atomicOr(&seen_bits[e_tok >> 5], 1u << (e_tok & 31)) >> (e_tok & 31)) & 1u);
        if (ngram > 0 && ngram <= cur && tid >= ngram - 1) {
          bool ban = true;
          for (int j = 0; j < ngram - 1; ++j)
            if (h[tid - ngram + 1 + j] != h[cur - ngram + 1 + j]) { ban = false; break; }
          if (ban) atomicOr(&ban_bits[e_tok >> 5], 1u << (e_tok & 31));
        }
      }
    }
    __syncthreads();
    if (own && e_tok != banned) {
      const uint32_t rb = reinterpret_cast<const unsigned short*>(x)[e_tok];
      if (bits_finite(rb)) {
        own_kr = (int)key_of(rb);
        const uint32_t eb = edit_bits(rb, theta);
        if (!((ban_bits[e_tok >> 5] >> (e_tok & 31)) & 1u) && bits_finite(eb)) own_ke = (int)key_of(eb);
      }
    }
  }
  // moves the owners' counts from the edited bins to the raw bins (dir = 1) or back (dir = 0): integer adds, any order gives the same words
  auto move_owned = [&](int dir) {
    const int from = dir ? own_ke : own_kr, to = dir ? own_kr : own_ke;
    if (from >= 0) atomicSub(&hist[(from >> 1) + (from >> 6)], 1u << ((from & 1) * 16));
    if (to >= 0) atomicAdd(&hist[(to >> 1) + (to >> 6)], 1u << ((to & 1) * 16));
  };

  // ---- sweep 1: the histogram of the candidates (finite, not the banned EOS column)
  for (int c = tid; c < nvec; c += SP_THREADS) {
    const u32x4 tv = *reinterpret_cast<const u32x4*>(x + (int64_t)c * 8);
    uint32_t seen8 = 0, ban8 = 0;                      // EDIT: the vector's 8 bits of the two maps
    if constexpr (EDIT) {
      seen8 = (seen_bits[c >> 2] >> ((c & 3) * 8)) & 0xFFu;
      if (seen8) ban8 = (ban_bits[c >> 2] >> ((c & 3) * 8)) & 0xFFu;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = c * 8 + e;
      uint32_t b = (tv[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
      if (col >= V) continue;
      if (!bits_finite(b)) {                           // NaN / +-inf: never a candidate; NaN or +inf spoil the row's log-softmax
        if (b != 0xFF80u) s_bad = 1;
        continue;
      }
      if (col == banned) { s_eos_x = __uint_as_float(b << 16); continue; }
      if (EDIT && ((seen8 >> e) & 1u)) {
        if ((ban8 >> e) & 1u) continue;
        b = edit_bits(b, theta);
        if (!bits_finite(b)) continue;                 // the penalised value overflowed bf16: no candidate
      }
      const uint32_t key = key_of(b), wd = key >> 1;
      atomicAdd(&hist[wd + (wd >> 5)], 1u << ((key & 1u) * 16));
    }
  }
  __syncthreads();

  // ---- pass A: candidates per thread (thread 0 holds the highest keys), the highest key
  const int chunk = SP_THREADS - 1 - tid;
  int n_t = 0, top_t = -1;
  walk_bins(hist, chunk, [&](int key, int cnt) { if (top_t < 0) top_t = key; n_t += cnt; return true; });
  int N;
  const int S_t = block_scan_i(n_t, sc, N);            // candidates in the bins above this thread's
  const int top_key = block_max_i(top_t, sc);

  if (N == 0) {                                        // no candidate at all: the row emits EOS and is finished
    if (tid == 0) {
      a.ids[out_i] = a.eos_token_id;
      a.done[r] = 1;
      if (a.u_out) a.u_out[r] = u;
      if (a.thr_out) a.thr_out[r] = INFINITY;
      if (a.kept_count_out) a.kept_count_out[r] = 0;
      if (a.kept_mass_out) a.kept_mass_out[r] = 0.f;
    }
    return;
  }

  // ---- top-k: the key of the k-th largest candidate; ties at it all stay (TopKLogitsWarper removes scores < kth)
  const int k = a.top_k;
  if (k > 0 && k < N) {
    if (S_t < k && k <= S_t + n_t) {
      int cum = S_t;
      walk_bins(hist, chunk, [&](int key, int cnt) {
        cum += cnt;
        if (cum >= k) { s_kth = key; s_cnt_ge = cum; return false; }
        return true;
      });
    }
  } else if (tid == 0) {
    s_cnt_ge = N;
  }
  __syncthreads();
  const int kth = s_kth;

  // ---- pass B: class masses over what top-k kept (z = x / temperature, relative to the top class), and the raw row's sum for
  // the model log-probability (temperature 1, every finite column, the banned EOS included)
  const float T = a.temperature;
  const float mz = val_of(top_key) / T;
  const float eos_x = s_eos_x;
  float mr = fmaxf(val_of(top_key), eos_x);
  float mass_t = 0.f, raw_t = 0.f;
  if (n_t > 0)
    walk_bins(hist, chunk, [&](int key, int cnt) {
      const float xv = val_of(key);
      if (!EDIT) raw_t += (float)cnt * __expf(xv - mr);
      if (key >= kth) mass_t += (float)cnt * __expf(xv / T - mz);
      return true;
    });
  float Zk, raw_sum;
  const float A_t = block_scan_f(mass_t, sc, Zk);      // mass of the classes above this thread's bins
  if constexpr (EDIT) {                                // the raw sum over the RAW histogram (every thread is past its walk: the scan's barriers)
    move_owned(1);
    __syncthreads();
    int rtop_t = -1;
    walk_bins(hist, chunk, [&](int key, int) { rtop_t = key; return false; });
    mr = fmaxf(val_of(block_max_i(rtop_t, sc)), eos_x);          // N > 0: the raw row has a finite column
    walk_bins(hist, chunk, [&](int key, int cnt) { raw_t += (float)cnt * __expf(val_of(key) - mr); return true; });
  }
  (void)block_scan_f(raw_t, sc, raw_sum);
  if constexpr (EDIT) {
    move_owned(0);
    __syncthreads();
  }
  raw_sum += __expf(eos_x - mr);                       // 0 when no column is banned
  const float lse = mr + logf(raw_sum);

  // ---- top-p: a class stays iff the mass of the strictly higher classes is < top_p * Zk.  The highest class that fails ends the
  // kept set, so the kept set is a threshold set whatever the rounding of the scan did between two threads.
  int fail_t = -1, fail_cnt = 0;
  float fail_cum = 0.f;
  if (a.top_p < 1.0f && n_t > 0) {
    const float P = a.top_p * Zk;
    float cum = A_t;
    int cc = S_t;
    walk_bins(hist, chunk, [&](int key, int cnt) {
      if (key < kth) return false;
      if (!(cum < P)) { fail_t = key; fail_cnt = cc; fail_cum = cum; return false; }
      cum += (float)cnt * __expf(val_of(key) / T - mz);
      cc += cnt;
      return true;
    });
  }
  const int F = block_max_i(fail_t, sc);
  if (F >= 0) {
    if (fail_t == F) { s_kept_cnt = fail_cnt; s_kept_mass = fail_cum; }
  } else if (tid == 0) {
    s_kept_cnt = s_cnt_ge; s_kept_mass = Zk;
  }
  __syncthreads();
  const float Zkept = s_kept_mass;
  const int floor_key = max(kth, F + 1);               // kept = candidates with key >= floor_key

  // ---- the draw: inverse CDF over the kept classes, highest first; inside a class the members are equal, so the member index is
  // a division.  The first class whose cumulative mass exceeds u * Zkept is the highest key that reports a hit.
  const float target = u * Zkept;
  int hit_t = -1, hit_j = 0, low_t = INT_MAX, low_cnt = 0;
  if (n_t > 0) {
    float cum = A_t;
    walk_bins(hist, chunk, [&](int key, int cnt) {
      if (key < floor_key) return false;
      low_t = key; low_cnt = cnt;
      const float e = __expf(val_of(key) / T - mz);
      if (hit_t < 0 && cum + (float)cnt * e > target) {
        hit_t = key;
        hit_j = e > 0.f ? min(max((int)floorf((target - cum) / e), 0), cnt - 1) : 0;
      }
      cum += (float)cnt * e;
      return true;
    });
  }
  const int H = block_max_i(hit_t, sc);
  const int L = -block_max_i(low_t == INT_MAX ? -INT_MAX : -low_t, sc);      // the lowest kept key
  if (H >= 0) {
    if (hit_t == H) { s_hit = H; s_hit_j = hit_j; }
  } else if (low_t == L) {                             // rounding left u * Zkept at or above the last cumulative mass: the last kept token
    s_hit = L; s_hit_j = low_cnt - 1;
  }
  __syncthreads();
  const int hit = s_hit, j = s_hit_j;

  // ---- sweep 2: the j-th column of the chosen class in ascending token order; thread t holds columns [t * per, (t + 1) * per)
  // the histogram key column `col` went under in sweep 1, -1 if it was no candidate
  auto member_key = [&](uint32_t b, uint32_t seen, uint32_t ban) -> int {
    if (!bits_finite(b)) return -1;
    if (EDIT && seen) {
      if (ban) return -1;
      b = edit_bits(b, theta);
      if (!bits_finite(b)) return -1;
    }
    return (int)key_of(b);
  };
  auto map8 = [&](const uint32_t* bits, int c) -> uint32_t { return EDIT ? (bits[c >> 2] >> ((c & 3) * 8)) & 0xFFu : 0u; };
  const int vpt = (nvec + SP_THREADS - 1) / SP_THREADS;
  u32x4 tv[SP_MAX_VEC];
  int c_t = 0;
#pragma unroll
  for (int i = 0; i < SP_MAX_VEC; ++i) {
    const int c = tid * vpt + i;
    if (i < vpt && c < nvec) {
      tv[i] = *reinterpret_cast<const u32x4*>(x + (int64_t)c * 8);
      const uint32_t seen8 = map8(seen_bits, c), ban8 = map8(ban_bits, c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = c * 8 + e;
        if (col < V && col != banned && member_key((tv[i][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu, (seen8 >> e) & 1u, (ban8 >> e) & 1u) == hit) ++c_t;
      }
    }
  }
  int n_hit;
  const int P_t = block_scan_i(c_t, sc, n_hit);
  if (P_t <= j && j < P_t + c_t) {
    int left = j - P_t, tok = -1;
#pragma unroll
    for (int i = 0; i < SP_MAX_VEC; ++i) {
      const int c = tid * vpt + i;
      if (i < vpt && c < nvec) {
        const uint32_t seen8 = map8(seen_bits, c), ban8 = map8(ban_bits, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int col = c * 8 + e;
          const uint32_t b = (tv[i][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
          if (col < V && col != banned && member_key(b, (seen8 >> e) & 1u, (ban8 >> e) & 1u) == hit) {
            if (left == 0 && tok < 0) { tok = col; s_raw_x = __uint_as_float(b << 16); }
            --left;
          }
        }
      }
    }
    s_tok = tok;
  }
  __syncthreads();

  if (tid == 0) {
    const int tok = s_tok;
    a.ids[out_i] = tok;
    if (tok == a.eos_token_id) a.done[r] = 1;
    a.seq_logprob[r] += s_bad ? NAN : ((EDIT ? s_raw_x : val_of(hit)) - lse);
    if (a.u_out) a.u_out[r] = u;
    if (a.thr_out) a.thr_out[r] = val_of(L);
    if (a.kept_count_out) a.kept_count_out[r] = s_kept_cnt;
    if (a.kept_mass_out) a.kept_mass_out[r] = Zkept / Zk;
  }
}

}  // namespace

namespace {
// the shared checks and the launch of ph_sample_step (edit = false) and ph_sample_step_edit
int sample_step_launch(const ph_sample_step_args* a, bool edit, float theta, int ngram, hipStream_t stream) {
  PH_CHECK_ARG(a && a->logits && a->ids && a->done && a->seq_logprob, "ph_sample_step: null pointer");
  PH_CHECK_ARG(a->V >= 8 && a->V <= 65535, "ph_sample_step: vocabulary %d outside 8..65535 (16-bit class counts)", a->V);
  PH_CHECK_ARG(a->ld >= a->V && (a->ld % 8) == 0 && (((uintptr_t)a->logits) & 15) == 0,
               "ph_sample_step: logit rows must be 16-byte aligned (ld %lld: a multiple of 8 elements, >= V)", (long long)a->ld);
  PH_CHECK_ARG(a->R >= 1 && a->rows_per_logit >= 1 && a->R % a->rows_per_logit == 0, "ph_sample_step: bad row count %d / rows per logit row %d", a->R,
               a->rows_per_logit);
  PH_CHECK_ARG(a->Tmax > 0 && a->cur >= 0 && a->cur < a->Tmax, "ph_sample_step: position %d outside 0..Tmax-1 (Tmax %d)", a->cur, a->Tmax);
  PH_CHECK_ARG(a->temperature > 0.f && a->temperature < INFINITY, "ph_sample_step: temperature must be a positive finite number");
  PH_CHECK_ARG(a->top_p > 0.f && a->top_p <= 1.f, "ph_sample_step: top_p outside (0, 1]");
  PH_CHECK_ARG(a->top_k >= 0, "ph_sample_step: top_k %d below 0", a->top_k);
  PH_CHECK_ARG(!a->ban_eos || (a->eos_token_id >= 0 && a->eos_token_id < a->V), "ph_sample_step: eos_token_id %d outside the vocabulary", a->eos_token_id);
  if (edit) {
    PH_CHECK_ARG(a->cur >= 1 && a->cur <= PH_EDIT_MAX_CUR, "ph_sample_step_edit: history length %d outside 1..%d", a->cur, PH_EDIT_MAX_CUR);
    PH_CHECK_ARG(theta > 0.f && theta < INFINITY, "ph_sample_step_edit: repetition_penalty must be a positive finite number");
    PH_CHECK_ARG(ngram >= 0, "ph_sample_step_edit: no_repeat_ngram_size %d below 0", ngram);
  }
  ProfScope prof__(PH_FAM_MISC, 0.0, 4.0 * a->R * (double)a->V, stream, "sample_step");
  if (!edit) {
    hipLaunchKernelGGL(sample_step_kernel<false>, dim3(a->R), dim3(SP_THREADS), 0, stream, *a, 1.0f, 0);
  } else {
    hipLaunchKernelGGL(sample_step_kernel<true>, dim3(a->R), dim3(SP_THREADS), 0, stream, *a, theta, ngram);
  }
  PH_LAUNCH_CHECK("sample_step_kernel");
  return PH_OK;
}
}  // namespace

extern "C" int ph_sample_step(const ph_sample_step_args* a, hipStream_t stream) { return sample_step_launch(a, false, 1.0f, 0, stream); }

extern "C" int ph_sample_step_edit(const ph_sample_step_args* a, float repetition_penalty, int no_repeat_ngram_size, hipStream_t stream) {
  return sample_step_launch(a, true, repetition_penalty, no_repeat_ngram_size, stream);
}
