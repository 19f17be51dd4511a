// Body of the bf16x3 attention kernels of sepr_attention.hip (relattn_x3_kernel and its packed-K form relattn_x3p_kernel), included INSIDE each
// __global__ function: it expects the constants DK, TRAIN, BP, ONE, NWV, PACK and the kernel parameters QKV, O, Tp, F, pe, maxlen, inv_sqrt_dk,
// lse, thr, dscale, seed, salt, pe_planes in scope.  Textual inclusion and not a __device__ template: hipcc optimises a device function on its
// own before it inlines it, and every existing instantiation then came out with commuted operands (three of them with other instruction
// counts); included, their device code is instruction for instruction that of the kernel before the packed form existed
// (profiles/attn_pack_device_code.txt).
  static_assert(!PACK || (DK == 16 && !TRAIN && !ONE), "the packed form is the dk = 16 inference kernel");
  static_assert(DK == 16 || DK == 32, "head width");
  // pe_planes (inference, round 4): the position table already split into bf16 hi / lo planes at pack time - the band rows of a key
  // tile are then copied global -> registers -> LDS as they are (half of this kernel's staged elements lose their VALU split)
  // BP is a template parameter: as a run-time flag every band fetch computed both tables' addresses and selected (16 VALU per key tile)
  static_assert(!(TRAIN && BP), "the training forward reads the fp32 table");
  // ONE (training forward of the plain-bf16 precision): operands rounded to bf16 once, one MFMA per product, no lo planes in LDS
  static_assert(TRAIN || !ONE, "inference keeps the split-fp32 products");
  constexpr bool bp = BP;
  DropKey dkey = {0u, 0u};
  if (TRAIN && thr) dkey = sepr_drop_key(seed, salt, 2u);
  static_assert(NWV == AT_NW, "waves (16-query slices) per workgroup");
  constexpr int NT = 64 * NWV;
  constexpr int QB = 16 * NWV, KT = 64;
  // K / band row stride in bf16 (DK used + 8 pad; DK = 16: the pad is the zero half of K = 32).  PACK: no pad - with 32-byte rows the 16 lanes
  // one ds_read_b128 cycle serves (8 of group g, 8 of group g + 1, 16 bytes further) tile the 64 banks exactly; 48-byte rows are 2-way there
  constexpr int KSB = PACK ? DK : DK + 8;
  constexpr int OT = DK / 16;         // 16-row tiles of O^T
  constexpr int NU = (KT * (DK / 4) + NT - 1) / NT;                       // K / V float4 per thread per key tile
  constexpr int NBU = ((QB + KT - 1) * (DK / 4) + NT - 1) / NT;             // band float4 per thread
  // V^T row stride in bf16 (144 B).  PACK: 136 B = 34 dwords, so the 16 rows one 8-byte fragment read covers start 2 banks apart (of 32)
  // instead of 4 (rows ii and ii + 8 on the same banks), and the four rows a staging thread group writes spread over 8-bank steps
  constexpr int VSB = PACK ? KT + 4 : KT + 8;
  constexpr int NBAND = QB + KT - 1;
  constexpr int PSK = 52;             // skew scratch row stride in floats (48 used)
  constexpr int LO = ONE ? 0 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 Kh[KT * KSB], Kl_[LO * KT * KSB + 8];
  __shared__ __attribute__((aligned(16))) __bf16 Vh[DK * VSB], Vl_[LO * DK * VSB + 8];
  __shared__ __attribute__((aligned(16))) __bf16 Bh[NBAND * KSB], Bl_[LO * NBAND * KSB + 8];
  __bf16* const Kl = ONE ? Kh : Kl_;          // ONE: dead aliases (the reads through them stay in bounds and feed nothing)
  __bf16* const Vl = ONE ? Vh : Vl_;
  __bf16* const Bl = ONE ? Bh : Bl_;
  __shared__ __attribute__((aligned(16))) float Psk[NWV * 16 * PSK];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ii = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * QB, h = blockIdx.y, seq = blockIdx.z;
  const int ld = 3 * F;
  const float* base = QKV + (long long)seq * Tp * ld + h * DK;
  const int i = i0 + 16 * w + ii;
  const bool active = i < Tp;
  const bool lowk = DK == 32 || g < 2;            // DK = 16: lane groups 2,3 carry the zero half of the K = 32 fragments:
  const int gk = DK == 32 ? g : (g & 1);          // they read the (zeroed) 8-element pad at the end of every K / band row
  // PACK: groups 2,3 read the same 8 channels as groups 0,1, of the lo plane; there is no pad
  const int go = PACK ? 8 * (g & 1) : (DK == 32 ? 8 * g : 8 * (g < 2 ? g : 2));
  if constexpr (!PACK) {
    for (int r = tid; r < KT; r += NT) {
#pragma unroll
      for (int e = DK; e < KSB; ++e) {
        Kh[r * KSB + e] = (__bf16)0.f;
        if constexpr (!ONE) Kl[r * KSB + e] = (__bf16)0.f;
      }
    }
    for (int r = tid; r < NBAND; r += NT) {
#pragma unroll
      for (int e = DK; e < KSB; ++e) {
        Bh[r * KSB + e] = (__bf16)0.f;
        if constexpr (!ONE) Bl[r * KSB + e] = (__bf16)0.f;
      }
    }
  }

  // B fragments of this lane's query (scaled), shared by the q.k and the q.band products
  bf16x8 qh, ql;
  {
    const float* qp = base + (long long)(active ? i : Tp - 1) * ld + 8 * gk;
    const float4 a = ld4(qp), b = ld4(qp + 4);
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (PACK) {   // the same 8 channels in all four lane groups: qh = [q_hi | q_hi], ql = [q_lo | q_lo] as K = 32 B fragments;
                              // the scale carries log2(e): the softmax below runs in base 2 (o / l does not depend on the base)
        const float v = x[e] * (inv_sqrt_dk * 1.44269504088896340736f);
        const __bf16 hh = (__bf16)v;
        qh[e] = hh;
        ql[e] = (__bf16)(v - (float)hh);
      } else {
        const float v = lowk ? x[e] * inv_sqrt_dk : 0.f;
        const __bf16 hh = (__bf16)v;
        qh[e] = hh;
        ql[e] = (__bf16)(v - (float)hh);
      }
    }
  }
  f32x4 o[OT];                                 // O^T[d = 16 t + 4g + r][query ii]
#pragma unroll
  for (int t = 0; t < OT; ++t) o[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float mrun = -1e30f, lrun = 0.f;
  float* const psk = Psk + (w * 16 + ii) * PSK;

  // staging registers: NU K and V float4 per thread (64 keys x DK) and NBU band float4 (127 rows x DK)
  float4 rk[NU], rv[NU], rb[NBU];
  auto fetch = [&](int j0) {          // global -> registers for the key tile starting at j0
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int idx = tid + NT * u;
      const int j = j0 + idx / (DK / 4), sc4 = idx % (DK / 4);
      rk[u] = zero4();
      rv[u] = zero4();
      if (j < Tp && (NT * NU == KT * (DK / 4) || idx < KT * (DK / 4))) {
        const float* kp = base + (long long)j * ld + F + 4 * sc4;
        rk[u] = ld4(kp);
        rv[u] = ld4(kp + F);
      }
    }
#pragma unroll
    for (int u = 0; u < NBU; ++u) {
      const int idx = tid + NT * u;
      const int rr = idx / (DK / 4) < NBAND ? idx / (DK / 4) : NBAND - 1;
      int rel = i0 - j0 - (KT - 1) + rr;                      // i - j for band row rr
      rel = rel < -maxlen ? -maxlen : (rel > maxlen - 1 ? maxlen - 1 : rel);
      const long long off = (long long)(rel + maxlen) * DK + 4 * (idx % (DK / 4));
      if (bp) {       // 4 bf16 of the hi plane in .x/.y, of the lo plane in .z/.w (bit patterns carried in the float4 registers)
        const uint2 hh = *reinterpret_cast<const uint2*>(pe_planes + off);
        const uint2 ll = *reinterpret_cast<const uint2*>(pe_planes + 2LL * maxlen * DK + off);
        rb[u] = make_float4(__uint_as_float(hh.x), __uint_as_float(hh.y), __uint_as_float(ll.x), __uint_as_float(ll.y));
      } else {
        rb[u] = ld4(pe + off);
      }
    }
  };
  fetch(0);
  for (int j0 = 0; j0 < Tp; j0 += KT) {
    __syncthreads();   // previous tile fully consumed
    // ---- registers -> LDS: K rows, V transposed and the band of the position table as bf16 hi / lo planes ----------
    {
      bf16x4 hh, ll;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int idx = tid + NT * u;
        const int sjj = idx / (DK / 4), sc4 = idx % (DK / 4);
        if (NT * NU > KT * (DK / 4) && idx >= KT * (DK / 4)) continue;
        split4(rk[u], hh, ll);
        *reinterpret_cast<bf16x4*>(Kh + sjj * KSB + 4 * sc4) = hh;
        if constexpr (!ONE) *reinterpret_cast<bf16x4*>(Kl + sjj * KSB + 4 * sc4) = ll;
        split4(rv[u], hh, ll);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          Vh[(4 * sc4 + e) * VSB + sjj] = hh[e];
          if constexpr (!ONE) Vl[(4 * sc4 + e) * VSB + sjj] = ll[e];
        }
      }
#pragma unroll
      for (int u = 0; u < NBU; ++u) {
        const int idx = tid + NT * u;
        if (idx < NBAND * (DK / 4)) {
          if (bp) {
            *reinterpret_cast<uint2*>(Bh + (idx / (DK / 4)) * KSB + 4 * (idx % (DK / 4))) = make_uint2(__float_as_uint(rb[u].x), __float_as_uint(rb[u].y));
            *reinterpret_cast<uint2*>(Bl + (idx / (DK / 4)) * KSB + 4 * (idx % (DK / 4))) = make_uint2(__float_as_uint(rb[u].z), __float_as_uint(rb[u].w));
          } else {
            split4(rb[u], hh, ll);
            *reinterpret_cast<bf16x4*>(Bh + (idx / (DK / 4)) * KSB + 4 * (idx % (DK / 4))) = hh;
            if constexpr (!ONE) *reinterpret_cast<bf16x4*>(Bl + (idx / (DK / 4)) * KSB + 4 * (idx % (DK / 4))) = ll;
          }
        }
      }
    }
    __syncthreads();
    if (j0 + KT < Tp) fetch(j0 + KT);   // the next tile's rows fly under this tile's arithmetic

    // ---- ONE online-softmax update per 64-key tile (round 4; one per 32 keys before): the scores of both 32-key pairs are formed
    //      first - two independent MFMA -> skew -> bias chains the scheduler can interleave - then one max / exchange / rescale
    //      round, then both P.V products.  Keys past Tp carry -1e30 (their V rows are staged as zeros), so a partial last tile
    //      simply runs both pairs.
    {
      float sv[2][2][4];
      if constexpr (PACK) {
        // A = [x_hi | x_lo]: lane groups 0,1 read 8 channels of the hi plane, groups 2,3 the SAME 8 channels of the lo plane - one LDS read
        // per K / band fragment (the unpacked arm reads two, half of each the zero pad).  With B = [q_hi | q_hi] and then [q_lo | q_lo] two
        // full MFMAs give the four-term split product x_hi.q_hi + x_lo.q_hi + x_hi.q_lo + x_lo.q_lo (three half-empty ones gave three
        // terms).  The band products of BOTH pairs come first (independent of everything else in the tile; the five distinct 16-row tiles
        // are computed once); a pair's skewed bias is then read back as the accumulator its score MFMAs START from.
        const __bf16* const Kx = g >= 2 ? Kl : Kh;
        const __bf16* const Bx = g >= 2 ? Bl : Bh;
        f32x4 bt[2][3];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int bb = 16 * w - 32 * p + 32;
#pragma unroll
          for (int tb = 0; tb < 3; ++tb) {
            const int row = bb + 16 * tb + (15 - ii);           // reversed inside the tile, clamped: as in the unpacked arm below
            const int rc = row < NBAND ? row : NBAND - 1;
            const bf16x8 bx = *reinterpret_cast<const bf16x8*>(Bx + rc * KSB + go);
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bx, qh, a, 0, 0, 0);
            bt[p][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bx, ql, a, 0, 0, 0);
          }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int tb = 0; tb < 3; ++tb)                         // mirrored store: see the unpacked arm
            st4(psk + 32 - 16 * tb + 4 * g, make_float4(bt[p][tb][0], bt[p][tb][1], bt[p][tb][2], bt[p][tb][3]));
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int b0 = ii + 31 - 16 * s - 4 * g;
            const int row = 32 * p + 16 * s + ii;
            const bf16x8 kx = *reinterpret_cast<const bf16x8*>(Kx + row * KSB + go);
            f32x4 a;
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = psk[47 - b0 + r];
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kx, qh, a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kx, ql, a, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) sv[p][s][r] = a[r];
          }
        }
      } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          // S^T[key = 16 s + 4g + r][query ii] for the two 16-key halves s
          f32x4 sc[2];
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int row = 32 * p + 16 * s + ii;
            const bf16x8 kh = *reinterpret_cast<const bf16x8*>(Kh + row * KSB + go);
            const bf16x8 kl = *reinterpret_cast<const bf16x8*>(Kl + row * KSB + go);
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh, a, 0, 0, 0);
            if constexpr (!ONE) {
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql, a, 0, 0, 0);
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh, a, 0, 0, 0);
            }
            sc[s] = a;
          }
          // relative-position term: P^T[b][query], band row of (query ql, key kl) is bb + b, b = ql - kl + 31
          const int bb = 16 * w - 32 * p + 32;
#pragma unroll
          for (int tb = 0; tb < 3; ++tb) {
            const int row = bb + 16 * tb + (15 - ii);             // <= 126 except unused rows of the last tile; REVERSED inside the 16-row tile:
                                                                  // the lane's four results are then band rows in DESCENDING order (see the store)
            const int rc = row < NBAND ? row : NBAND - 1;
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bh + rc * KSB + go);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bl + rc * KSB + go);
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, qh, a, 0, 0, 0);
            if constexpr (!ONE) {
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ql, a, 0, 0, 0);
              a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, qh, a, 0, 0, 0);
            }
            // a[r] = band row b = 16 tb + 15 - 4g - r of this query, stored MIRRORED (row b at float 47 - b = 32 - 16 tb + 4g + r): the four
            // bias values of a key group are then read in ASCENDING address order, i.e. as register pairs in the order of the score pairs they
            // are added to.  With the rows in natural order hipcc packed that add as v_pk_add_f32 op_sel:[0,1] op_sel_hi:[1,0] (pair swap) -
            // the gfx950-faulty form of sepr_common.h norm4_pinned: THAT was round 4's "nondeterministic mask pass" (tools/isa_lint.py now
            // rejects the form; reversing the band rows in the A fragment costs nothing, reversing the results would cost v_pk_mov's)
            st4(psk + 32 - 16 * tb + 4 * g, make_float4(a[0], a[1], a[2], a[3]));
          }
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int b0 = ii + 31 - 16 * s - 4 * g;              // b of key 16 s + 4g + 0; r steps down
            float bias[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bias[r] = psk[47 - b0 + r];  // unconditional: the reads issue back to back
#pragma unroll
            for (int r = 0; r < 4; ++r)
              sv[p][s][r] = sc[s][r] + bias[r];
          }
        }
      }
      // only a tile that reaches past Tp pays the 16 key-bound selects: ONE wave-uniform pass (as selects inside the loop above they cost 48
      // VALU per tile and hipcc turned four of the bias reads into exec-masked blocks with their own LDS waits: 300 -> 212 VALU per full
      // tile).  Round 4 withdrew this form as "run-to-run nondeterministic, cause not established"; round 5 established it - not the pass
      // but the packed bias add the compiler formed around it (see the mirrored store above).
      if (j0 + KT > Tp) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (j0 + 32 * p + 16 * s + 4 * g + r >= Tp) sv[p][s][r] = -1e30f;
      }
      float mx = -1e30f;
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          mx = fmaxf(mx, fmaxf(fmaxf(sv[p][s][0], sv[p][s][1]), fmaxf(sv[p][s][2], sv[p][s][3])));
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(mrun, mx);
      const float corr = PACK ? __builtin_amdgcn_exp2f(mrun - mnew) : __expf(mrun - mnew);
      bf16x8 ph[2], pl[2];
      float psum = 0.f;
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = PACK ? __builtin_amdgcn_exp2f(sv[p][s][r] - mnew) : __expf(sv[p][s][r] - mnew);
            psum += pv;
            const __bf16 hh = (__bf16)pv;
            ph[p][4 * s + r] = hh;
            pl[p][4 * s + r] = (__bf16)(pv - (float)hh);
          }
      if (TRAIN && thr) {   // dropped probabilities for the PV product only; keys 16 s + 4g + {0,1} / {2,3} are the element pairs
        const unsigned row = (unsigned)((seq * gridDim.y + h) * Tp + i);
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const unsigned jp = (unsigned)(j0 + 32 * p + 16 * s + 4 * g) >> 1;
            const unsigned d0 = sepr_drop_word(dkey, row, jp), d1 = sepr_drop_word(dkey, row, jp + 1u);
            const bool k0 = (d0 & 0xffffu) >= thr, k1 = (d0 >> 16) >= thr, k2 = (d1 & 0xffffu) >= thr, k3 = (d1 >> 16) >= thr;
            if (!k0) { ph[p][4 * s] = (__bf16)0.f; pl[p][4 * s] = (__bf16)0.f; }
            if (!k1) { ph[p][4 * s + 1] = (__bf16)0.f; pl[p][4 * s + 1] = (__bf16)0.f; }
            if (!k2) { ph[p][4 * s + 2] = (__bf16)0.f; pl[p][4 * s + 2] = (__bf16)0.f; }
            if (!k3) { ph[p][4 * s + 3] = (__bf16)0.f; pl[p][4 * s + 3] = (__bf16)0.f; }
          }
      }
      lrun = lrun * corr + psum;
      mrun = mnew;
      // ---- O^T[d][query] += V^T[d][key slots] . P[key slots][query]; slot e -> key 16 (e / 4) + 4g + e % 4 --------
#pragma unroll
      for (int t = 0; t < OT; ++t) {
        o[t][0] *= corr; o[t][1] *= corr; o[t][2] *= corr; o[t][3] *= corr;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const __bf16* vh0 = Vh + (16 * t + ii) * VSB + 32 * p + 4 * g;
          const __bf16* vl0 = Vl + (16 * t + ii) * VSB + 32 * p + 4 * g;
          const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(vh0), a1 = *reinterpret_cast<const bf16x4*>(vh0 + 16);
          const bf16x4 b0v = *reinterpret_cast<const bf16x4*>(vl0), b1v = *reinterpret_cast<const bf16x4*>(vl0 + 16);
          const bf16x8 vh = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
          const bf16x8 vl = {b0v[0], b0v[1], b0v[2], b0v[3], b1v[0], b1v[1], b1v[2], b1v[3]};
          o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph[p], o[t], 0, 0, 0);
          if constexpr (!ONE) {
            o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl[p], o[t], 0, 0, 0);
            o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl, ph[p], o[t], 0, 0, 0);
          }
        }
      }
    }
  }
  float ltot = lrun + __shfl_xor(lrun, 16, 64);
  ltot += __shfl_xor(ltot, 32, 64);
  if (active) {
    const float inv = (TRAIN ? dscale : 1.0f) / ltot;
#pragma unroll
    for (int t = 0; t < OT; ++t)
      st4(O + ((long long)seq * Tp + i) * F + h * DK + 16 * t + 4 * g,
          make_float4(o[t][0] * inv, o[t][1] * inv, o[t][2] * inv, o[t][3] * inv));
    if (TRAIN && lse && g == 0) lse[((long long)seq * gridDim.y + h) * Tp + i] = mrun + logf(ltot);
  }
