// attn.hip — causal flash attention fwd/bwd for gfx950 (CDNA4 MFMA).
//
// Replaces torch SDPA inside the reference's Llama forward
// (attn_implementation "sdpa", reference train_fsdp.py:107; called via
// model(**batch) at train_fsdp.py:378 / train_diloco_torch.py:313) and its
// autograd backward (train_fsdp.py:383).
//
// Design (MI355X-first, correctness-first structure for round 1):
//  - mfma_f32_16x16x32_{bf16,f16} tiles; 4 waves (256 thr) per workgroup.
//  - forward: workgroup owns 64 q rows of one (b, h); waves own 16 q rows
//    each; K/V staged in LDS by all 256 threads (K row-major [32][D+8] for
//    direct B-fragment ds_read_b128, V transposed [D][32+8] at staging time
//    so PV B-fragments are contiguous reads); online softmax in fp32 with
//    running (m, l) per row, wave-shuffle row reductions (no serial lanes);
//    P goes through a small per-wave LDS tile to re-shape C-layout ->
//    A-layout.  lse = m + log(l) saved for backward.
//  - backward: split into a dK/dV kernel (grid over kv tiles, key on the
//    MFMA lane) and a dQ kernel (grid over q tiles, query on the lane);
//    P/dS recomputed from lse and kept in registers — no atomics anywhere,
//    so gradients are bit-deterministic run to run (the reference's tests
//    compare loss traces, test_train.py:82).  GQA handled by writing dK/dV
//    per q-head; the caller sums the group (ratio == 1 writes directly).
//
// MFMA fragment maps used (verified on hardware by dk_probe_mfma_16x16x32,
// tests/test_gpu_ops.py::test_mfma_probe):
//   A[16][32]: lane l holds row = l&15,  k = 8*(l>>4) + j   (j = 0..7)
//   B[32][16]: lane l holds col = l&15,  k = 8*(l>>4) + j
//   C[16][16]: lane l holds col = l&15,  row = (l>>4)*4 + r (r = 0..3)

#include "dk_common.h"
#include "../../include/diloco_kernels.h"

#include <math.h>
#include <stdlib.h>

typedef __attribute__((ext_vector_type(8))) _Float16 halfx8;

template <int DT> struct MFMA16;
template <> struct MFMA16<2> {
  using frag = shortx8;
  static __device__ __forceinline__ floatx4 mma(frag a, frag b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct MFMA16<1> {
  using frag = halfx8;
  static __device__ __forceinline__ floatx4 mma(frag a, frag b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// gfx950 hardware transpose-read: within each 16-lane group, the lanes
// supply the 8-byte chunks of a [4 rows][16 cols] bf16/f16 tile and lane L
// receives column L&15: out[j] = tile[row j][col L&15].  Lane addresses are
// independent, so the tile rows may live at ANY stride — a 16x16x32 MFMA
// B-fragment can be read straight from a ROW-MAJOR LDS image (two reads:
// k = 8g..8g+3 and 8g+4..8g+7, g = lane>>4), eliminating the separate
// transposed staging image and its 8 scalar LDS writes per thread.
// Chunk->lane semantics hardware-verified (tools: tr16_probe).
template <int DT> struct TrRead;
template <> struct TrRead<2> {
  typedef __attribute__((ext_vector_type(4))) __bf16 v4;
  static __device__ __forceinline__ void rd(const unsigned short* p, void* out) {
    v4 r = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) v4*)(uintptr_t)(const void*)p);
    __builtin_memcpy(out, &r, 8);
  }
};
template <> struct TrRead<1> {
  typedef __attribute__((ext_vector_type(4))) __fp16 v4;
  static __device__ __forceinline__ void rd(const _Float16* p, void* out) {
    v4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
        (__attribute__((address_space(3))) v4*)(uintptr_t)(const void*)p);
    __builtin_memcpy(out, &r, 8);
  }
};
// B-fragment (16x16x32 map: lane l -> col l&15, k = 8*(l>>4)+j) from a
// row-major image img[row][ds]: rows row0.., cols col0..col0+15.
template <int DT>
__device__ __forceinline__ typename MFMA16<DT>::frag trread_bfrag(
    const typename DTraits<DT>::T* img, int row0, int col0, int ds, int lane) {
  const int rb = row0 + 8 * (lane >> 4) + ((lane & 15) >> 2);
  const int cb = col0 + 4 * (lane & 3);
  typename MFMA16<DT>::frag f;
  TrRead<DT>::rd(img + rb * ds + cb, &f);
  TrRead<DT>::rd(img + (rb + 4) * ds + cb, (char*)&f + 8);
  return f;
}

// 4-wide 16-bit vector store (one ds_write_b64) for the packed P/dS images
template <int DT> struct Pack4;
template <> struct Pack4<2> { using V = shortx4; };
template <> struct Pack4<1> { typedef __attribute__((ext_vector_type(4))) _Float16 V; };

#define NEG_BIG (-1e30f)

// row-group shuffle reduce: combine over the 16 lanes that share l>>4
__device__ __forceinline__ float grp16_max(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, DK_WAVE));
  return x;
}
__device__ __forceinline__ float grp16_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, DK_WAVE);
  return x;
}

// ======================= forward =======================
// v2 structure (guide T14/T3/T5): KT=64 kv tiles, double-buffered LDS, async
// register staging (next tile's global loads issued before compute, written
// to the other LDS buffer after it — HBM latency hides under MFMA), ONE
// barrier per tile, both K and V staged ROW-MAJOR (PV fragments are
// transposed at read time by ds_read_b64_tr_b16), s_setprio(1) around the
// MFMA clusters.
// LDS: K[2][KT][DS] | V[2][KT][DS] | P[4][16][KS]

template <int DT, int D>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    typename DTraits<DT>::T* __restrict__ o, float* __restrict__ lse,
    const typename DTraits<DT>::T* __restrict__ q,
    const typename DTraits<DT>::T* __restrict__ k,
    const typename DTraits<DT>::T* __restrict__ v,
    int B, int Hq, int Hkv, int S, float scale,
    int64_t o_sb, int64_t o_sh, int64_t o_sr,
    int64_t v_sb, int64_t v_sh, int64_t v_sr) {
  using TR = DTraits<DT>;
  using T = typename TR::T;
  using MF = MFMA16<DT>;
  using frag = typename MF::frag;
  constexpr int KT = 64;           // kv tile
  constexpr int KS = KT + 8;       // padded LDS stride (keys dim), u16 units
  constexpr int DS = D + 8;        // padded LDS stride (channel dim)
  constexpr int NKC = D / 32;      // mfma K-chunks over channels
  constexpr int NDN = D / 16;      // output channel tiles
  constexpr int NNT = KT / 16;     // 16-key sub-tiles per kv tile
  constexpr int LPT = (KT * D) / 8 / 256;  // b128 loads per thread per tile

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* K_lds = (T*)smem_raw;                       // [2][KT][DS]
  T* V_lds = K_lds + 2 * KT * DS;                // [2][KT][DS] row-major
  T* P_lds = V_lds + 2 * KT * DS;                // [4][16][KS]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo = lane & 15;        // col index (key / d-channel)
  const int hi = lane >> 4;        // k-chunk group & row group

  const int nQT = (S + 63) / 64;
  int bid = blockIdx.x;
  const int qt = bid % nQT;
  const int h = (bid / nQT) % Hq;
  const int b = bid / (nQT * Hq);
  const int hkv = h / (Hq / Hkv);

  const int q0 = qt * 64 + wave * 16;            // this wave's first q row
  const int64_t qoff = (((int64_t)b * Hq + h) * S) * D;
  const int64_t kvoff = (((int64_t)b * Hkv + hkv) * S) * D;
  const int64_t voff = v_sb ? ((int64_t)b * v_sb + (int64_t)hkv * v_sh) : kvoff;
  const int64_t v_rs = v_sb ? v_sr : (int64_t)D;

  // Q A-fragments for this wave's 16 rows (clamped on the tail tile)
  frag q_frag[NKC];
  {
    const int qrow = q0 + lo;
    const int qr_c = qrow < S ? qrow : S - 1;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
      q_frag[kc] = *(const frag*)(q + qoff + (int64_t)qr_c * D + kc * 32 + hi * 8);
  }

  float m_run[4], l_run[4];
  floatx4 o_acc[NDN];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = NEG_BIG; l_run[r] = 0.f; }
#pragma unroll
  for (int dn = 0; dn < NDN; ++dn) o_acc[dn] = (floatx4)(0.f);

  const int kv_end = min(S, qt * 64 + 64);       // causal upper bound
  const int n_kt = (kv_end + KT - 1) / KT;

  // staging registers (async split): this thread's pieces of the next tile
  frag kreg[LPT], vreg[LPT];
  const int st_row[2] = {(int)threadIdx.x / (D / 8), (int)(threadIdx.x + 256) / (D / 8)};
  const int st_c8[2] = {((int)threadIdx.x % (D / 8)) * 8, ((int)(threadIdx.x + 256) % (D / 8)) * 8};

  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int krow = kt * KT + st_row[i];
      const int kr_c = krow < S ? krow : S - 1;
      kreg[i] = *(const frag*)(k + kvoff + (int64_t)kr_c * D + st_c8[i]);
      vreg[i] = *(const frag*)(v + voff + (int64_t)kr_c * v_rs + st_c8[i]);
    }
  };
  auto write_tile = [&](int buf) {
    T* Kb = K_lds + buf * KT * DS;
    T* Vb = V_lds + buf * KT * DS;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      *(frag*)(Kb + st_row[i] * DS + st_c8[i]) = kreg[i];
      *(frag*)(Vb + st_row[i] * DS + st_c8[i]) = vreg[i];
    }
  };

  load_tile(0);
  write_tile(0);
  __syncthreads();

  for (int kt = 0; kt < n_kt; ++kt) {
    const int kbase = kt * KT;
    const int cur = kt & 1;
    T* Kb = K_lds + cur * KT * DS;
    T* Vb = V_lds + cur * KT * DS;
    if (kt + 1 < n_kt) load_tile(kt + 1);  // async: in flight during compute

    // ---- S tile = Q K^T (16 q x KT keys) ----
    floatx4 sc[NNT];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt) {
      sc[nt] = (floatx4)(0.f);
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        frag bk = *(const frag*)(Kb + (nt * 16 + lo) * DS + kc * 32 + hi * 8);
        sc[nt] = MF::mma(q_frag[kc], bk, sc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- mask + online softmax over KT keys ----
    // tiles strictly below the diagonal and fully in-bounds need no
    // per-element mask (wave-uniform branch; saves 2 cmp+sel per element)
    const bool full_tile = (kbase + KT <= q0) && (kbase + KT <= S);
    float p[NNT][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0 + hi * 4 + r;
      float rm = NEG_BIG;
      float sv[NNT];
      if (full_tile) {
#pragma unroll
        for (int nt = 0; nt < NNT; ++nt) {
          sv[nt] = sc[nt][r] * scale;
          rm = fmaxf(rm, sv[nt]);
        }
      } else {
#pragma unroll
        for (int nt = 0; nt < NNT; ++nt) {
          const int kk = kbase + nt * 16 + lo;
          sv[nt] = (kk > qrow || kk >= S) ? NEG_BIG : sc[nt][r] * scale;
          rm = fmaxf(rm, sv[nt]);
        }
      }
      rm = grp16_max(rm);
      const float m_new = fmaxf(m_run[r], rm);
      const float alpha = __expf(m_run[r] - m_new);
      float psum = 0.f;
#pragma unroll
      for (int nt = 0; nt < NNT; ++nt) {
        p[nt][r] = sv[nt] <= NEG_BIG ? 0.f : __expf(sv[nt] - m_new);
        psum += p[nt][r];
      }
      l_run[r] = l_run[r] * alpha + grp16_sum(psum);
      m_run[r] = m_new;
#pragma unroll
      for (int dn = 0; dn < NDN; ++dn) o_acc[dn][r] *= alpha;
    }

    // ---- P through per-wave LDS: C-layout -> A-layout ----
    T* Pw = P_lds + wave * 16 * KS;
#pragma unroll
    for (int nt = 0; nt < NNT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Pw[(hi * 4 + r) * KS + nt * 16 + lo] = TR::fromF(p[nt][r]);
    // same-wave LDS dependency: compiler inserts lgkmcnt waits
    frag pa[KT / 32];
#pragma unroll
    for (int c = 0; c < KT / 32; ++c)
      pa[c] = *(const frag*)(Pw + lo * KS + c * 32 + hi * 8);

    // ---- O += P V ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dn = 0; dn < NDN; ++dn)
#pragma unroll
      for (int c = 0; c < KT / 32; ++c) {
        frag bv = trread_bfrag<DT>(Vb, c * 32, dn * 16, DS, lane);
        o_acc[dn] = MF::mma(pa[c], bv, o_acc[dn]);
      }
    __builtin_amdgcn_s_setprio(0);

    if (kt + 1 < n_kt) write_tile((kt + 1) & 1);  // T14: write late, after compute
    __syncthreads();
  }

  // ---- epilogue ----
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + hi * 4 + r;
    if (qrow >= S) continue;
    const float inv_l = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    const int64_t obase = (int64_t)b * o_sb + (int64_t)h * o_sh + (int64_t)qrow * o_sr;
#pragma unroll
    for (int dn = 0; dn < NDN; ++dn)
      o[obase + dn * 16 + lo] = TR::fromF(o_acc[dn][r] * inv_l);
    if (lo == 0) lse[((int64_t)b * Hq + h) * S + qrow] = m_run[r] + __logf(l_run[r]);
  }
}

// ======================= forward v3: swapped QK^T, in-register softmax =======================
// 32x32x16 MFMA tiles.  S^T = mfma(K, Q) puts 16 of a q-row's 32 key-scores
// in ONE lane (q = lane&31; the other 16 in the partner lane l^32), so the
// softmax row reduction is an in-lane tree + ONE shfl_xor(32) — no 16-lane
// shuffle chains, no P LDS round trip: P is packed to bf16 in-register
// (cvt_pk pairs) and redistributed with permlane32_swap into the PV B-frag
// (layouts + swap semantics hardware-verified by dk_probe_mfma_32x32x16 and
// dk_probe_permlane32).  PV computes O^T = mfma(V^T, P) so the accumulator
// stays q-lane-local (alpha rescale in-lane).  Wave owns 32 q rows; LDS is
// only the double-buffered K/V^T tiles (same async staging as v2).
typedef __attribute__((ext_vector_type(16))) float floatx16;
typedef __attribute__((ext_vector_type(4))) int intx4;

template <int DT> struct MFMA32;
template <> struct MFMA32<2> {
  using frag = shortx8;
  static __device__ __forceinline__ floatx16 mma(frag a, frag b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct MFMA32<1> {
  using frag = halfx8;
  static __device__ __forceinline__ floatx16 mma(frag a, frag b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// A-fragment for 32x32x16 MFMA (map: lane l -> row l&31, k = 8*(l>>5)+j)
// transposed out of a ROW-MAJOR image img[k][ds] via ds_read_b64_tr_b16:
// out[j] = img[row0 + 8*(l>>5) + j][col0 + (l&31)].  The four 16-lane tr
// groups split as (k-half = l>>5) x (col-half = (l>>4)&1).
template <int DT>
__device__ __forceinline__ typename MFMA32<DT>::frag trread_afrag32(
    const typename DTraits<DT>::T* img, int row0, int col0, int ds, int lane) {
  const int lam = lane & 15;
  const int rb = row0 + 8 * (lane >> 5) + (lam >> 2);
  const int cb = col0 + 16 * ((lane >> 4) & 1) + 4 * (lam & 3);
  typename MFMA32<DT>::frag f;
  TrRead<DT>::rd(img + rb * ds + cb, &f);
  TrRead<DT>::rd(img + (rb + 4) * ds + cb, (char*)&f + 8);
  return f;
}

// Pack rows 16c .. 16c+15 of a 32x32 f32 accumulator X (C map: col = l&31,
// row = (r&3) + 8*(r>>2) + 4*(l>>5)) into a 32x32x16 fragment in natural k
// order: element j of lane half h = X[16c + 8h + j][l&31] — the B operand of
// A·X (or the A operand of X^T·B).  Registers 8c..8c+7 hold rows
// {0..3, 8..11} + 4h of the chunk; cvt_pk pairs them as w0=(0,1) w1=(2,3)
// w2=(8,9) w3=(10,11) (+4 in the high half), and swap(w0,w2) ->
// dwords {0, 2}, swap(w1,w3) -> {1, 3} regroups them (hardware-verified by
// dk_probe_mfma_32x32x16 and dk_probe_permlane32).
template <int DT> struct Pack2;
template <> struct Pack2<2> { typedef __attribute__((ext_vector_type(2))) __bf16 V; };
template <> struct Pack2<1> { typedef __attribute__((ext_vector_type(2))) _Float16 V; };
// two f32 -> one packed 16-bit dword: a single v_cvt_pk_{bf16,f16}_f32 (RTNE)
template <int DT>
__device__ __forceinline__ unsigned cvt_pk2(float a, float b) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  typename Pack2<DT>::V r = __builtin_convertvector((f2){a, b}, typename Pack2<DT>::V);
  unsigned u;
  __builtin_memcpy(&u, &r, 4);
  return u;
}

template <int DT>
__device__ __forceinline__ typename MFMA32<DT>::frag pack_frag32(const floatx16& x, int c) {
  const int base = c * 8;
  const unsigned w0 = cvt_pk2<DT>(x[base + 0], x[base + 1]);
  const unsigned w1 = cvt_pk2<DT>(x[base + 2], x[base + 3]);
  const unsigned w2 = cvt_pk2<DT>(x[base + 4], x[base + 5]);
  const unsigned w3 = cvt_pk2<DT>(x[base + 6], x[base + 7]);
  auto s0 = __builtin_amdgcn_permlane32_swap((int)w0, (int)w2, false, false);
  auto s1 = __builtin_amdgcn_permlane32_swap((int)w1, (int)w3, false, false);
  intx4 pw;
  pw[0] = s0[0];
  pw[1] = s1[0];
  pw[2] = s0[1];
  pw[3] = s1[1];
  return *(typename MFMA32<DT>::frag*)&pw;
}

template <int DT, int D>
__global__ __launch_bounds__(256, 4) void attn_fwd_v3_kernel(
    typename DTraits<DT>::T* __restrict__ o, float* __restrict__ lse,
    const typename DTraits<DT>::T* __restrict__ q,
    const typename DTraits<DT>::T* __restrict__ k,
    const typename DTraits<DT>::T* __restrict__ v,
    int B, int Hq, int Hkv, int S, float scale,
    int64_t o_sb, int64_t o_sh, int64_t o_sr,
    int64_t v_sb, int64_t v_sh, int64_t v_sr) {
  using TR = DTraits<DT>;
  using T = typename TR::T;
  using MF = MFMA32<DT>;
  using frag = typename MF::frag;
  constexpr int KT = 64;            // kv tile (2 x 32-key subtiles)
  constexpr int KS = KT + 8;        // P image stride (u16)
  constexpr int DS = D + 8;         // K image stride
  constexpr int NKC = D / 16;       // 16-channel contraction chunks for QK^T
  constexpr int NMT = D / 32;       // 32-row d tiles for O^T
  constexpr int LPT = (KT * D) / 8 / 256;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* K_lds = (T*)smem_raw;                       // [2][KT][DS]
  T* V_lds = K_lds + 2 * KT * DS;                // [2][KT][DS] row-major

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo32 = lane & 31;       // q row within the wave
  const int hi5 = lane >> 5;

  const int nQT = (S + 127) / 128;
  int bid = blockIdx.x;
  const int qt = bid % nQT;
  const int h = (bid / nQT) % Hq;
  const int b = bid / (nQT * Hq);
  const int hkv = h / (Hq / Hkv);

  const int q0 = qt * 128 + wave * 32;           // wave's first q row
  const int qrow = q0 + lo32;                    // this lane's q row
  const int64_t qoff = (((int64_t)b * Hq + h) * S) * D;
  const int64_t kvoff = (((int64_t)b * Hkv + hkv) * S) * D;
  const int64_t voff = v_sb ? ((int64_t)b * v_sb + (int64_t)hkv * v_sh) : kvoff;
  const int64_t v_rs = v_sb ? v_sr : (int64_t)D;

  // persistent Q B-fragments: slot j of chunk kc = Q[qrow][kc*16 + hi5*8 + j]
  frag q_frag[NKC];
  {
    const int qr_c = qrow < S ? qrow : S - 1;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
      q_frag[kc] = *(const frag*)(q + qoff + (int64_t)qr_c * D + kc * 16 + hi5 * 8);
  }

  float m_run = NEG_BIG, l_run = 0.f;
  floatx16 oacc[NMT];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) oacc[mt] = (floatx16)(0.f);

  const int kv_end = min(S, qt * 128 + 128);
  const int n_kt = (kv_end + KT - 1) / KT;

  // async double-buffered staging (same structure as v2)
  shortx8 kreg[LPT], vreg[LPT];
  const int st_row[2] = {(int)threadIdx.x / (D / 8), (int)(threadIdx.x + 256) / (D / 8)};
  const int st_c8[2] = {((int)threadIdx.x % (D / 8)) * 8, ((int)(threadIdx.x + 256) % (D / 8)) * 8};

  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int krow = kt * KT + st_row[i];
      const int kr_c = krow < S ? krow : S - 1;
      kreg[i] = *(const shortx8*)(k + kvoff + (int64_t)kr_c * D + st_c8[i]);
      vreg[i] = *(const shortx8*)(v + voff + (int64_t)kr_c * v_rs + st_c8[i]);
    }
  };
  auto write_tile = [&](int buf) {
    T* Kb = K_lds + buf * KT * DS;
    T* Vb = V_lds + buf * KT * DS;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      *(shortx8*)(Kb + st_row[i] * DS + st_c8[i]) = kreg[i];
      *(shortx8*)(Vb + st_row[i] * DS + st_c8[i]) = vreg[i];
    }
  };

  load_tile(0);
  write_tile(0);
  __syncthreads();

  for (int kt = 0; kt < n_kt; ++kt) {
    const int kbase = kt * KT;
    const int cur = kt & 1;
    T* Kb = K_lds + cur * KT * DS;
    T* Vb = V_lds + cur * KT * DS;
    if (kt + 1 < n_kt) load_tile(kt + 1);

#pragma unroll
    for (int st = 0; st < 2; ++st) {            // two 32-key subtiles
      const int sbase = kbase + st * 32;
      // wave-uniform diagonal skip: keys all above this wave's q rows would
      // be fully masked (rm = NEG_BIG -> alpha 1, psum 0: state unchanged).
      if (sbase >= q0 + 32) continue;
      // ---- S^T = K Q^T ----
      floatx16 sc = (floatx16)(0.f);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        frag ka = *(const frag*)(Kb + (st * 32 + lo32) * DS + kc * 16 + hi5 * 8);
        sc = MF::mma(ka, q_frag[kc], sc);
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- in-lane online softmax for q row `qrow` (p values live in the
      // sc accumulator registers: no extra p[] array) ----
      const bool full_tile = (sbase + 32 <= q0) && (sbase + 32 <= S);
      float rm = NEG_BIG;
      if (full_tile) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[r] *= scale;
          rm = fmaxf(rm, sc[r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = sbase + (r & 3) + 8 * (r >> 2) + 4 * hi5;
          sc[r] = (key > qrow || key >= S) ? NEG_BIG : sc[r] * scale;
          rm = fmaxf(rm, sc[r]);
        }
      }
      rm = fmaxf(rm, __shfl_xor(rm, 32, DK_WAVE));
      const float m_new = fmaxf(m_run, rm);
      const float alpha = __expf(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[r] = sc[r] <= NEG_BIG ? 0.f : __expf(sc[r] - m_new);
        psum += sc[r];
      }
      psum += __shfl_xor(psum, 32, DK_WAVE);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[mt][r] *= alpha;

      // ---- pack P into PV B-fragments (chunk c = keys sbase + c*16 ..) ----
      frag pfrag[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) pfrag[c] = pack_frag32<DT>(sc, c);

      // ---- O^T += V^T P  (A = V^T tr_read from row-major V, B = P) ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          frag va = trread_afrag32<DT>(Vb, st * 32 + c * 16, mt * 32, DS,
                                       (int)(threadIdx.x & 63));
          oacc[mt] = MF::mma(va, pfrag[c], oacc[mt]);
        }
      __builtin_amdgcn_s_setprio(0);
    }

    if (kt + 1 < n_kt) write_tile((kt + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: lane q = lo32 owns its whole row of O^T ----
  if (qrow < S) {
    const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
    const int64_t obase = (int64_t)b * o_sb + (int64_t)h * o_sh + (int64_t)qrow * o_sr;
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi5;
        o[obase + d] = TR::fromF(oacc[mt][r] * inv_l);
      }
    if (hi5 == 0) lse[((int64_t)b * Hq + h) * S + qrow] = m_run + __logf(l_run);
  }
}

// ======================= bwd preprocess: delta = rowsum(do*o) =======================
// each wave covers WR=4 rows per iteration: 16 lanes per row, shortx4 loads
// (8 B/lane), 4-lane... 16-lane-group shuffle reduce per row
template <int DT>
__global__ void attn_bwd_pre_kernel(float* __restrict__ delta,
                                    const typename DTraits<DT>::T* __restrict__ do_,
                                    const typename DTraits<DT>::T* __restrict__ o,
                                    int64_t rows, int H, int S, int D,
                                    int64_t g_sb, int64_t g_sh, int64_t g_sr) {
  using TR = DTraits<DT>;
  using T = typename TR::T;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;   // lo: D-quad index, hi: row-in-group
  const int64_t w0 = (int64_t)blockIdx.x * 4 + wave;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const int quads = D / 4;  // shortx4 chunks per row (D in {32, 64})
  const int64_t groups = (rows + 3) / 4;
  for (int64_t g = w0; g < groups; g += stride) {  // 4 rows per wave-iteration
    const int64_t r = g * 4 + hi;
    const int64_t rc = r < rows ? r : rows - 1;
    const int sp = (int)(rc % S);
    const int hh = (int)((rc / S) % H);
    const int64_t b = rc / ((int64_t)S * H);
    const int64_t base = b * g_sb + hh * g_sh + sp * g_sr;
    float s = 0.f;
    for (int q4 = lo; q4 < quads; q4 += 16) {
      shortx4 dv = *(const shortx4*)(do_ + base + q4 * 4);
      shortx4 ov = *(const shortx4*)(o + base + q4 * 4);
      float df[4], of[4];
      packed_to_f32<DT, 4>(&dv, df);
      packed_to_f32<DT, 4>(&ov, of);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += df[j] * of[j];
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, DK_WAVE);
    if (lo == 0 && r < rows) delta[r] = s;
  }
}

// ======================= bwd: key/query on the lane, 32x32x16 tiles =======================
// Both backward kernels orient every score tile so the accumulator of S and
// dP is already the B operand of the product that follows it (guide
// Appendix B "Key on the lane"): pack_frag32 (cvt_pk + permlane32_swap)
// turns the f32 tile into bf16/f16 fragments in registers, so neither
// kernel writes P or dS to LDS.  Row constants ride in the accumulators:
// S starts at -lse/scale, so p = exp2(S * scale*log2(e)) is one multiply and
// one v_exp; dP starts at -delta, so dS = p * dP is one multiply.  scale is
// applied once to dQ / dK in the epilogue.  The causal mask runs only on the
// diagonal tile (and the <S bound only on the last), chosen wave-uniformly,
// so off-diagonal tiles carry no compares.  No atomics: every output element
// is written by exactly one lane (bit-deterministic run to run).

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// 8-byte store of four consecutive f32 accumulator rows (r = 4g .. 4g+3 of
// the 32x32 C map, rows 8g + 4*(l>>5) + 0..3) as one packed 16-bit vector.
template <int DT>
__device__ __forceinline__ void store4(typename DTraits<DT>::T* dst, const floatx16& x,
                                       int g, float mul) {
  using P4 = typename Pack4<DT>::V;
  P4 pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) ((typename DTraits<DT>::T*)&pk)[i] = DTraits<DT>::fromF(x[4 * g + i] * mul);
  *(P4*)dst = pk;
}

// dQ: grid over (b, hq, q-tile of 128); 4 waves x 32 q rows.  Structurally
// the v3 forward with K in place of V and dS in place of P:
//   S^T = mfma(K, Q), dP^T = mfma(V, dO)   (q = lane&31, 16 keys per lane)
//   dQ^T += K^T dS^T                        (A = K^T tr_read from row-major K)
// LDS: K[2][64][D+8] | V[2][64][D+8], async double-buffered.
template <int DT, int D>
__global__ __launch_bounds__(256, 3) void attn_bwd_dq_kernel(
    typename DTraits<DT>::T* __restrict__ dq_out,
    const typename DTraits<DT>::T* __restrict__ do_,
    const typename DTraits<DT>::T* __restrict__ q,
    const typename DTraits<DT>::T* __restrict__ k,
    const typename DTraits<DT>::T* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    int B, int Hq, int Hkv, int S, float scale,
    int64_t g_sb, int64_t g_sh, int64_t g_sr,
    int64_t v_sb, int64_t v_sh, int64_t v_sr) {
  using TR = DTraits<DT>;
  using T = typename TR::T;
  using MF = MFMA32<DT>;
  using frag = typename MF::frag;
  constexpr int KT = 64;            // staged kv tile (2 x 32-key subtiles)
  constexpr int DS = D + 8;
  constexpr int NKC = D / 16;       // 16-deep contraction chunks for S^T, dP^T
  constexpr int NMT = D / 32;       // 32-row d tiles of dQ^T
  constexpr int LPT = (KT * D) / 8 / 256;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* K_lds = (T*)smem_raw;                       // [2][KT][DS]
  T* V_lds = K_lds + 2 * KT * DS;                // [2][KT][DS]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo32 = lane & 31;
  const int hi5 = lane >> 5;

  const int nQT = (S + 127) / 128;
  int bid = blockIdx.x;
  const int qt = bid % nQT;
  const int h = (bid / nQT) % Hq;
  const int b = bid / (nQT * Hq);
  const int hkv = h / (Hq / Hkv);

  const int q0 = qt * 128 + wave * 32;
  const int qrow = q0 + lo32;
  const int64_t qoff = (((int64_t)b * Hq + h) * S) * D;
  const int64_t kvoff = (((int64_t)b * Hkv + hkv) * S) * D;
  const int64_t lseoff = ((int64_t)b * Hq + h) * S;
  const int64_t voff = v_sb ? ((int64_t)b * v_sb + (int64_t)hkv * v_sh) : kvoff;
  const int64_t v_rs = v_sb ? v_sr : (int64_t)D;
  const int64_t gbase = (int64_t)b * g_sb + (int64_t)h * g_sh;

  // Q / dO B-fragments: slot j of chunk kc = X[qrow][kc*16 + hi5*8 + j]
  frag q_frag[NKC], do_frag[NKC];
  float nl2, dl_q;   // -lse*log2(e), delta of this lane's row
  {
    const int qr_c = qrow < S ? qrow : S - 1;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      q_frag[kc] = *(const frag*)(q + qoff + (int64_t)qr_c * D + kc * 16 + hi5 * 8);
      do_frag[kc] = *(const frag*)(do_ + gbase + (int64_t)qr_c * g_sr + kc * 16 + hi5 * 8);
    }
    nl2 = -lse[lseoff + qr_c] * 1.4426950408889634f;
    dl_q = delta[lseoff + qr_c];
  }
  const float c2 = scale * 1.4426950408889634f;  // scale * log2(e)

  floatx16 dq_acc[NMT];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) dq_acc[mt] = (floatx16)(0.f);

  const int kv_end = min(S, qt * 128 + 128);
  const int n_kt = (kv_end + KT - 1) / KT;

  shortx8 kreg[LPT], vreg[LPT];
  int st_row[LPT], st_c8[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    st_row[i] = (int)(threadIdx.x + 256 * i) / (D / 8);
    st_c8[i] = ((int)(threadIdx.x + 256 * i) % (D / 8)) * 8;
  }
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int krow = kt * KT + st_row[i];
      const int kr_c = krow < S ? krow : S - 1;
      kreg[i] = *(const shortx8*)(k + kvoff + (int64_t)kr_c * D + st_c8[i]);
      vreg[i] = *(const shortx8*)(v + voff + (int64_t)kr_c * v_rs + st_c8[i]);
    }
  };
  auto write_tile = [&](int buf) {
    T* Kb = K_lds + buf * KT * DS;
    T* Vb = V_lds + buf * KT * DS;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      *(shortx8*)(Kb + st_row[i] * DS + st_c8[i]) = kreg[i];
      *(shortx8*)(Vb + st_row[i] * DS + st_c8[i]) = vreg[i];
    }
  };

  load_tile(0);
  write_tile(0);
  __syncthreads();

  for (int kt = 0; kt < n_kt; ++kt) {
    const int cur = kt & 1;
    const T* Kb = K_lds + cur * KT * DS;
    const T* Vb = V_lds + cur * KT * DS;
    if (kt + 1 < n_kt) load_tile(kt + 1);

#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int sbase = kt * KT + st * 32;
      if (sbase >= q0 + 32) continue;            // wave-uniform: fully masked
      floatx16 sc = (floatx16)(0.f), dp = (floatx16)(0.f);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        frag ka = *(const frag*)(Kb + (st * 32 + lo32) * DS + kc * 16 + hi5 * 8);
        sc = MF::mma(ka, q_frag[kc], sc);
        frag va = *(const frag*)(Vb + (st * 32 + lo32) * DS + kc * 16 + hi5 * 8);
        dp = MF::mma(va, do_frag[kc], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // dS^T in dp.  Off the diagonal every key (< sbase + 32 <= q0) is
      // below every q row of the wave, and for a valid row (< S) every such
      // key is valid too: no compares.  Rows >= S only feed their own
      // (unstored) dQ^T column.
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] = (dp[r] - dl_q) * exp2_fast(fmaf(sc[r], c2, nl2));
      if (sbase >= q0) {                       // diagonal subtile only
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = sbase + (r & 3) + 8 * (r >> 2) + 4 * hi5;
          if (key > qrow) dp[r] = 0.f;
        }
      }
      frag dsf[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) dsf[c] = pack_frag32<DT>(dp, c);

      // ---- dQ^T += K^T dS^T  (A = K^T tr_read from the row-major K image) ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          frag ka = trread_afrag32<DT>(Kb, st * 32 + c * 16, mt * 32, DS, lane);
          dq_acc[mt] = MF::mma(ka, dsf[c], dq_acc[mt]);
        }
      __builtin_amdgcn_s_setprio(0);
    }

    if (kt + 1 < n_kt) write_tile((kt + 1) & 1);
    __syncthreads();
  }

  // lane q = lo32 owns its row of dQ^T: d = mt*32 + 8g + 4*hi5 + 0..3
  if (qrow < S) {
    T* dst = dq_out + qoff + (int64_t)qrow * D;
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) store4<DT>(dst + mt * 32 + 8 * g + 4 * hi5, dq_acc[mt], g, scale);
  }
}

// dK/dV: grid over (b, hq, kv-tile of 128 keys); 4 waves x 32 keys.  The
// workgroup sweeps q tiles of 64 (two 32-row compute halves per barrier):
//   S = mfma(Q, K), dP = mfma(dO, V)       (key = lane&31, 16 q rows per lane)
//   dV^T += dO^T P,  dK^T += Q^T dS         (A = dO^T / Q^T tr_read from the
//                                            row-major staged images)
// K/V B-fragments stay in registers for the whole sweep.  The per-row
// constants (-lse/scale, -delta) are staged next to Q/dO and loaded straight
// into the S / dP accumulators (4 x ds_read_b128 each per half).
// LDS: Q[2][64][D+8] | dO[2][64][D+8] | lse'[2][64] f32 | -delta[2][64] f32
template <int DT, int D>
__global__ __launch_bounds__(256, 3) void attn_bwd_dkdv_kernel(
    typename DTraits<DT>::T* __restrict__ dk_out,
    typename DTraits<DT>::T* __restrict__ dv_out,
    const typename DTraits<DT>::T* __restrict__ do_,
    const typename DTraits<DT>::T* __restrict__ q,
    const typename DTraits<DT>::T* __restrict__ k,
    const typename DTraits<DT>::T* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    int B, int Hq, int Hkv, int S, float scale,
    int64_t g_sb, int64_t g_sh, int64_t g_sr,
    int64_t v_sb, int64_t v_sh, int64_t v_sr,
    int64_t dv_sb, int64_t dv_sh, int64_t dv_sr) {
  using TR = DTraits<DT>;
  using T = typename TR::T;
  using MF = MFMA32<DT>;
  using frag = typename MF::frag;
  constexpr int QT = 32;                     // compute half (q rows)
  constexpr int QTT = 32;                    // staged tile (one per barrier)
  constexpr int DS = D + 8;
  constexpr int NKC = D / 16;
  constexpr int NMT = D / 32;
  constexpr int NCH = (QTT * D) / 8;         // 16-byte staging pieces per tensor
  constexpr int LPT = (NCH + 255) / 256;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* Q_lds = (T*)smem_raw;                   // [2][QTT][DS]
  T* dO_lds = Q_lds + 2 * QTT * DS;          // [2][QTT][DS]
  float* lse_lds = (float*)(dO_lds + 2 * QTT * DS);  // [2][QTT]  -lse/scale
  float* dl_lds = lse_lds + 2 * QTT;                 // [2][QTT]  -delta

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo32 = lane & 31;
  const int hi5 = lane >> 5;

  const int nKT = (S + 127) / 128;
  int bid = blockIdx.x;
  const int kt = bid % nKT;
  const int h = (bid / nKT) % Hq;
  const int b = bid / (nKT * Hq);
  const int hkv = h / (Hq / Hkv);

  const int k0 = kt * 128 + wave * 32;       // this wave's first key
  const int key = k0 + lo32;                 // this lane's key
  const int64_t qoff = (((int64_t)b * Hq + h) * S) * D;
  const int64_t kvoff = (((int64_t)b * Hkv + hkv) * S) * D;
  const int64_t lseoff = ((int64_t)b * Hq + h) * S;
  const int64_t voff = v_sb ? ((int64_t)b * v_sb + (int64_t)hkv * v_sh) : kvoff;
  const int64_t v_rs = v_sb ? v_sr : (int64_t)D;
  const int64_t gbase = (int64_t)b * g_sb + (int64_t)h * g_sh;

  // K / V B-fragments: slot j of chunk kc = X[key][kc*16 + hi5*8 + j]
  frag k_frag[NKC], v_frag[NKC];
  {
    const int kr_c = key < S ? key : S - 1;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      k_frag[kc] = *(const frag*)(k + kvoff + (int64_t)kr_c * D + kc * 16 + hi5 * 8);
      v_frag[kc] = *(const frag*)(v + voff + (int64_t)kr_c * v_rs + kc * 16 + hi5 * 8);
    }
  }
  const float c2 = scale * 1.4426950408889634f;

  floatx16 dv_acc[NMT], dk_acc[NMT];
#pragma unroll
  for (int mt = 0; mt < NMT; ++mt) { dv_acc[mt] = (floatx16)(0.f); dk_acc[mt] = (floatx16)(0.f); }

  const int qstart = (kt * 128) / QTT;
  const int nQT2 = (S + QTT - 1) / QTT;

  shortx8 qreg[LPT], dreg[LPT];
  float lse_reg = 0.f, dl_reg = 0.f;
  int st_row[LPT], st_c8[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    st_row[i] = (int)(threadIdx.x + 256 * i) / (D / 8);
    st_c8[i] = ((int)(threadIdx.x + 256 * i) % (D / 8)) * 8;
  }
  const int st_t = (int)threadIdx.x;
  auto load_qtile = [&](int qt) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      if (NCH % 256 && (int)threadIdx.x + 256 * i >= NCH) break;
      const int qr = qt * QTT + st_row[i];
      const int qr_c = qr < S ? qr : S - 1;
      qreg[i] = *(const shortx8*)(q + qoff + (int64_t)qr_c * D + st_c8[i]);
      dreg[i] = *(const shortx8*)(do_ + gbase + (int64_t)qr_c * g_sr + st_c8[i]);
    }
    if (st_t < QTT) {
      const int rr = qt * QTT + st_t;
      const int rr_c = rr < S ? rr : S - 1;
      lse_reg = -lse[lseoff + rr_c] / scale;
      dl_reg = -delta[lseoff + rr_c];
    }
  };
  auto write_qtile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      if (NCH % 256 && (int)threadIdx.x + 256 * i >= NCH) break;
      *(shortx8*)(Q_lds + buf * QTT * DS + st_row[i] * DS + st_c8[i]) = qreg[i];
      *(shortx8*)(dO_lds + buf * QTT * DS + st_row[i] * DS + st_c8[i]) = dreg[i];
    }
    if (st_t < QTT) {
      lse_lds[buf * QTT + st_t] = lse_reg;
      dl_lds[buf * QTT + st_t] = dl_reg;
    }
  };

  load_qtile(qstart);
  write_qtile(0);
  __syncthreads();

  for (int qt = qstart; qt < nQT2; ++qt) {
    const int cur = (qt - qstart) & 1;
    if (qt + 1 < nQT2) load_qtile(qt + 1);

#pragma unroll
    for (int hf = 0; hf < QTT / QT; ++hf) {
      const int qbase = qt * QTT + hf * QT;
      if (qbase + QT <= k0) continue;        // wave-uniform: every q < every key
      const T* Qb = Q_lds + cur * QTT * DS + hf * QT * DS;
      const T* dOb = dO_lds + cur * QTT * DS + hf * QT * DS;
      const float* lse_b = lse_lds + cur * QTT + hf * QT;
      const float* dl_b = dl_lds + cur * QTT + hf * QT;

      // row constants into the accumulators: register r is q row
      // 8*(r>>2) + 4*hi5 + (r&3)
      floatx16 sc, dp;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const floatx4 l4 = *(const floatx4*)(lse_b + 8 * g + 4 * hi5);
        const floatx4 d4 = *(const floatx4*)(dl_b + 8 * g + 4 * hi5);
#pragma unroll
        for (int i = 0; i < 4; ++i) { sc[4 * g + i] = l4[i]; dp[4 * g + i] = d4[i]; }
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        frag qa = *(const frag*)(Qb + lo32 * DS + kc * 16 + hi5 * 8);
        sc = MF::mma(qa, k_frag[kc], sc);
        frag doa = *(const frag*)(dOb + lo32 * DS + kc * 16 + hi5 * 8);
        dp = MF::mma(doa, v_frag[kc], dp);
      }
      __builtin_amdgcn_s_setprio(0);

      // P in sc, dS in dp.  Full tile: every q row >= every key of the wave
      // and < S.  Otherwise (diagonal / last tile) mask per element; keys
      // >= S need no mask: their dK/dV rows are never stored.
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = exp2_fast(sc[r] * c2);
      if (qbase < k0 + QT || qbase + QT > S) {   // diagonal / last tile only
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qr = qbase + (r & 3) + 8 * (r >> 2) + 4 * hi5;
          if (key > qr || qr >= S) sc[r] = 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] *= sc[r];
      frag pf[2], dsf[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        pf[c] = pack_frag32<DT>(sc, c);
        dsf[c] = pack_frag32<DT>(dp, c);
      }

      // ---- dV^T += dO^T P,  dK^T += Q^T dS ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          frag da = trread_afrag32<DT>(dOb, c * 16, mt * 32, DS, lane);
          dv_acc[mt] = MF::mma(da, pf[c], dv_acc[mt]);
          frag qa = trread_afrag32<DT>(Qb, c * 16, mt * 32, DS, lane);
          dk_acc[mt] = MF::mma(qa, dsf[c], dk_acc[mt]);
        }
      __builtin_amdgcn_s_setprio(0);
    }

    if (qt + 1 < nQT2) write_qtile(cur ^ 1);
    __syncthreads();
  }

  // lane key = lo32 owns its rows of dK^T / dV^T: d = mt*32 + 8g + 4*hi5 + 0..3
  // (per q-head layout [B,Hq,S,D]; caller sums GQA groups)
  if (key < S) {
    const int64_t dvoff = dv_sb ? ((int64_t)b * dv_sb + (int64_t)h * dv_sh) : qoff;
    const int64_t dv_rs = dv_sb ? dv_sr : (int64_t)D;
    T* dkp = dk_out + qoff + (int64_t)key * D;
    T* dvp = dv_out + dvoff + (int64_t)key * dv_rs;
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        store4<DT>(dkp + mt * 32 + 8 * g + 4 * hi5, dk_acc[mt], g, scale);
        store4<DT>(dvp + mt * 32 + 8 * g + 4 * hi5, dv_acc[mt], g, 1.f);
      }
  }
}

// ======================= C-ABI wrappers =======================

static bool use_attn_v2() {
  static int cached = -1;
  if (cached < 0) {
    const char* e = getenv("DK_ATTN_V2");
    cached = (e && e[0] == '1') ? 1 : 0;
  }
  return cached == 1;
}

template <int DT, int D>
static int launch_attn_fwd(void* o, float* lse, const void* q, const void* k,
                           const void* v, int64_t B, int64_t Hq, int64_t Hkv,
                           int64_t S, float scale, int64_t o_sb, int64_t o_sh,
                           int64_t o_sr, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                           dkStream stream) {
  using T = typename DTraits<DT>::T;
  constexpr int KT = 64, KS = KT + 8, DS = D + 8;
  if (!use_attn_v2()) {
    // v3: swapped QK^T, in-register softmax, 128 q rows per workgroup
    const int nQT = (int)((S + 127) / 128);
    const int grid = (int)(B * Hq * nQT);
    const size_t lds = sizeof(T) * (2 * KT * DS + 2 * KT * DS);
    hipLaunchKernelGGL((attn_fwd_v3_kernel<DT, D>), dim3(grid), dim3(256), lds,
                       (hipStream_t)stream, (T*)o, lse, (const T*)q, (const T*)k,
                       (const T*)v, (int)B, (int)Hq, (int)Hkv, (int)S, scale,
                       o_sb, o_sh, o_sr, v_sb, v_sh, v_sr);
    DK_CHECK_LAUNCH();
    return 0;
  }
  const int nQT = (int)((S + 63) / 64);
  const int grid = (int)(B * Hq * nQT);
  const size_t lds = sizeof(T) * (2 * KT * DS + 2 * KT * DS + 4 * 16 * KS);
  hipLaunchKernelGGL((attn_fwd_kernel<DT, D>), dim3(grid), dim3(256), lds,
                     (hipStream_t)stream, (T*)o, lse, (const T*)q, (const T*)k,
                     (const T*)v, (int)B, (int)Hq, (int)Hkv, (int)S, scale,
                     o_sb, o_sh, o_sr, v_sb, v_sh, v_sr);
  DK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dk_attn_fwd(void* o, float* lse, const void* q, const void* k,
                           const void* v, int64_t B, int64_t Hq, int64_t Hkv,
                           int64_t S, int64_t D, float scale,
                           int64_t o_sb, int64_t o_sh, int64_t o_sr,
                           int64_t v_sb, int64_t v_sh, int64_t v_sr, int dtype,
                           dkStream stream) {
  if (dtype != 1 && dtype != 2) return (int)hipErrorInvalidValue;
  if (o_sb == 0) { o_sb = Hq * S * D; o_sh = S * D; o_sr = D; }  // BHSD default
  if (D == 64) {
    if (dtype == 2) return launch_attn_fwd<2, 64>(o, lse, q, k, v, B, Hq, Hkv, S, scale, o_sb, o_sh, o_sr, v_sb, v_sh, v_sr, stream);
    return launch_attn_fwd<1, 64>(o, lse, q, k, v, B, Hq, Hkv, S, scale, o_sb, o_sh, o_sr, v_sb, v_sh, v_sr, stream);
  } else if (D == 32) {
    if (dtype == 2) return launch_attn_fwd<2, 32>(o, lse, q, k, v, B, Hq, Hkv, S, scale, o_sb, o_sh, o_sr, v_sb, v_sh, v_sr, stream);
    return launch_attn_fwd<1, 32>(o, lse, q, k, v, B, Hq, Hkv, S, scale, o_sb, o_sh, o_sr, v_sb, v_sh, v_sr, stream);
  }
  return (int)hipErrorInvalidValue;
}

extern "C" int dk_attn_bwd_preprocess(float* delta, const void* do_, const void* o,
                                      int64_t B, int64_t H, int64_t S, int64_t D,
                                      int64_t g_sb, int64_t g_sh, int64_t g_sr,
                                      int dtype, dkStream stream) {
  const int64_t rows = B * H * S;
  if (g_sb == 0) { g_sb = H * S * D; g_sh = S * D; g_sr = D; }
  int64_t g = (rows + 3) / 4;  // 4 waves per block, one row per wave-iteration
  int grid = (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
  DK_DISPATCH_DT(dtype, {
    if constexpr (kDT != 0) {
      using T = typename DTraits<kDT>::T;
      hipLaunchKernelGGL((attn_bwd_pre_kernel<kDT>), dim3(grid), dim3(256), 0,
                         (hipStream_t)stream, delta, (const T*)do_, (const T*)o,
                         rows, (int)H, (int)S, (int)D, g_sb, g_sh, g_sr);
    } else {
      return (int)hipErrorInvalidValue;
    }
  });
  DK_CHECK_LAUNCH();
  return 0;
}

template <int DT, int D>
static int launch_attn_bwd_dkdv(void* dk_o, void* dv_o, const void* do_, const void* q,
                                const void* k, const void* v, const float* lse,
                                const float* delta, int64_t B, int64_t Hq, int64_t Hkv,
                                int64_t S, float scale, int64_t g_sb, int64_t g_sh,
                                int64_t g_sr, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                                int64_t dv_sb, int64_t dv_sh, int64_t dv_sr,
                                dkStream stream) {
  using T = typename DTraits<DT>::T;
  constexpr int QTT = 32, DS = D + 8;
  // the epilogue stores 4 d-channels (8 B) per lane
  if (((uintptr_t)dv_o & 7) || (dv_sb | dv_sh | dv_sr) & 3) return (int)hipErrorInvalidValue;
  const int nKT = (int)((S + 127) / 128);    // 4 waves x 32 keys
  const int grid = (int)(B * Hq * nKT);
  const size_t lds = sizeof(T) * (4 * QTT * DS) + sizeof(float) * 4 * QTT;
  hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DT, D>), dim3(grid), dim3(256), lds,
                     (hipStream_t)stream, (T*)dk_o, (T*)dv_o, (const T*)do_,
                     (const T*)q, (const T*)k, (const T*)v, lse, delta,
                     (int)B, (int)Hq, (int)Hkv, (int)S, scale, g_sb, g_sh, g_sr,
                     v_sb, v_sh, v_sr, dv_sb, dv_sh, dv_sr);
  DK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dk_attn_bwd_dkdv(void* dk_o, void* dv_o, const void* do_, const void* q,
                                const void* k, const void* v, const float* lse,
                                const float* delta, int64_t B, int64_t Hq, int64_t Hkv,
                                int64_t S, int64_t D, float scale,
                                int64_t g_sb, int64_t g_sh, int64_t g_sr,
                                int64_t v_sb, int64_t v_sh, int64_t v_sr,
                                int64_t dv_sb, int64_t dv_sh, int64_t dv_sr, int dtype,
                                dkStream stream) {
  if (dtype != 1 && dtype != 2) return (int)hipErrorInvalidValue;
  if (g_sb == 0) { g_sb = Hq * S * D; g_sh = S * D; g_sr = D; }
  if (D == 64) {
    if (dtype == 2) return launch_attn_bwd_dkdv<2, 64>(dk_o, dv_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, dv_sb, dv_sh, dv_sr, stream);
    return launch_attn_bwd_dkdv<1, 64>(dk_o, dv_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, dv_sb, dv_sh, dv_sr, stream);
  } else if (D == 32) {
    if (dtype == 2) return launch_attn_bwd_dkdv<2, 32>(dk_o, dv_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, dv_sb, dv_sh, dv_sr, stream);
    return launch_attn_bwd_dkdv<1, 32>(dk_o, dv_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, dv_sb, dv_sh, dv_sr, stream);
  }
  return (int)hipErrorInvalidValue;
}

template <int DT, int D>
static int launch_attn_bwd_dq(void* dq_o, const void* do_, const void* q, const void* k,
                              const void* v, const float* lse, const float* delta,
                              int64_t B, int64_t Hq, int64_t Hkv, int64_t S,
                              float scale, int64_t g_sb, int64_t g_sh, int64_t g_sr,
                              int64_t v_sb, int64_t v_sh, int64_t v_sr,
                              dkStream stream) {
  using T = typename DTraits<DT>::T;
  constexpr int KT = 64, DS = D + 8;
  const int nQT = (int)((S + 127) / 128);    // 4 waves x 32 q rows
  const int grid = (int)(B * Hq * nQT);
  const size_t lds = sizeof(T) * (4 * KT * DS);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<DT, D>), dim3(grid), dim3(256), lds,
                     (hipStream_t)stream, (T*)dq_o, (const T*)do_, (const T*)q,
                     (const T*)k, (const T*)v, lse, delta, (int)B, (int)Hq,
                     (int)Hkv, (int)S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr);
  DK_CHECK_LAUNCH();
  return 0;
}

extern "C" int dk_attn_bwd_dq(void* dq_o, const void* do_, const void* q, const void* k,
                              const void* v, const float* lse, const float* delta,
                              int64_t B, int64_t Hq, int64_t Hkv, int64_t S, int64_t D,
                              float scale, int64_t g_sb, int64_t g_sh, int64_t g_sr,
                              int64_t v_sb, int64_t v_sh, int64_t v_sr,
                              int dtype, dkStream stream) {
  if (dtype != 1 && dtype != 2) return (int)hipErrorInvalidValue;
  if (g_sb == 0) { g_sb = Hq * S * D; g_sh = S * D; g_sr = D; }
  if (D == 64) {
    if (dtype == 2) return launch_attn_bwd_dq<2, 64>(dq_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, stream);
    return launch_attn_bwd_dq<1, 64>(dq_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, stream);
  } else if (D == 32) {
    if (dtype == 2) return launch_attn_bwd_dq<2, 32>(dq_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, stream);
    return launch_attn_bwd_dq<1, 32>(dq_o, do_, q, k, v, lse, delta, B, Hq, Hkv, S, scale, g_sb, g_sh, g_sr, v_sb, v_sh, v_sr, stream);
  }
  return (int)hipErrorInvalidValue;
}

// ======================= MFMA layout probe (test-only) =======================
// D = A[16][32] x B[32][16] using the fragment maps above; out is [16][16]
// f32 row-major.  A/B given row-major bf16.  The GPU test feeds asymmetric
// random matrices and compares with a host matmul (guide §5.4 rule 16).
__global__ void probe_mfma_kernel(float* __restrict__ out,
                                  const unsigned short* __restrict__ a,
                                  const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int lo = lane & 15, hi = lane >> 4;
  shortx8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ((unsigned short*)&af)[j] = a[lo * 32 + hi * 8 + j];        // A[row=lo][k=8*hi+j]
    ((unsigned short*)&bf)[j] = b[(hi * 8 + j) * 16 + lo];      // B[k=8*hi+j][col=lo]
  }
  floatx4 c = (floatx4)(0.f);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(hi * 4 + r) * 16 + lo] = c[r];  // C[row=(hi*4+r)][col=lo]
}

extern "C" int dk_probe_mfma_16x16x32_bf16(float* out_d, const void* a16x32,
                                           const void* b32x16, dkStream stream) {
  hipLaunchKernelGGL(probe_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     out_d, (const unsigned short*)a16x32, (const unsigned short*)b32x16);
  DK_CHECK_LAUNCH();
  return 0;
}

// Alternative candidate mapping (k interleaved: k = (l>>4) + 4*j) — a
// diagnostic twin so one GPU round can identify the true layout if the
// primary assumption fails.
__global__ void probe_mfma_alt_kernel(float* __restrict__ out,
                                      const unsigned short* __restrict__ a,
                                      const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int lo = lane & 15, hi = lane >> 4;
  shortx8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ((unsigned short*)&af)[j] = a[lo * 32 + (hi + 4 * j)];
    ((unsigned short*)&bf)[j] = b[(hi + 4 * j) * 16 + lo];
  }
  floatx4 c = (floatx4)(0.f);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(hi * 4 + r) * 16 + lo] = c[r];
}

extern "C" int dk_probe_mfma_16x16x32_bf16_alt(float* out_d, const void* a16x32,
                                               const void* b32x16, dkStream stream) {
  hipLaunchKernelGGL(probe_mfma_alt_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     out_d, (const unsigned short*)a16x32, (const unsigned short*)b32x16);
  DK_CHECK_LAUNCH();
  return 0;
}

// 32x32x16 bf16 probe — assumed maps:
//   A[32][16]: lane holds row = l&31, k = 8*(l>>5) + j (j = 0..7)
//   B[16][32]: lane holds col = l&31, k = 8*(l>>5) + j
//   C[32][32]: lane holds col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5)
typedef __attribute__((ext_vector_type(16))) float floatx16;
__global__ void probe_mfma32_kernel(float* __restrict__ out,
                                    const unsigned short* __restrict__ a,
                                    const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int lo = lane & 31, hi = lane >> 5;
  shortx8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ((unsigned short*)&af)[j] = a[lo * 16 + hi * 8 + j];
    ((unsigned short*)&bf)[j] = b[(hi * 8 + j) * 32 + lo];
  }
  floatx16 c = (floatx16)(0.f);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    out[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + lo] = c[r];
}

extern "C" int dk_probe_mfma_32x32x16_bf16(float* out_d, const void* a32x16,
                                           const void* b16x32, dkStream stream) {
  hipLaunchKernelGGL(probe_mfma32_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     out_d, (const unsigned short*)a32x16, (const unsigned short*)b16x32);
  DK_CHECK_LAUNCH();
  return 0;
}

// permlane32_swap semantics probe: in a[lane] = lane, b[lane] = 100+lane;
// writes the two results so the host can read the exact lane exchange.
__global__ void probe_permlane_kernel(int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  int a = lane, b = 100 + lane;
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  out[lane] = r[0];
  out[64 + lane] = r[1];
}

extern "C" int dk_probe_permlane32(int* out_d, dkStream stream) {
  hipLaunchKernelGGL(probe_permlane_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out_d);
  DK_CHECK_LAUNCH();
  return 0;
}
