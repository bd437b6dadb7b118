// zk_pairing_impl.hpp -- the pairing kernel and its call bodies, over the twist's curve type C
// (BN254_G2: zk_pairing_bn.hip, BLS381_G2: zk_pairing_bls.hip).
//
// Replaces <C>_pairing_affine = final_expo(miller_loop) (bls12_381_pairing.c, bn128_pairing.c) per row.  The
// value f^((p^12 - 1)/r) of the Miller function of the reference's loop is a canonical Fp12 element, so the
// rows are bit-equal without following the reference's schedule (tools/gen_pairing_prog.py: the formulas,
// the exponent identities and the addition chains).
//
// One kernel, k_pair_vm: an interpreter of (op | d << 8 | a << 16 | b << 24) words over the lane's Fp2 cells
// (zk_tower.hpp).  The streams (zk_pairing_prog.inc) are flat -- the Miller loop's 64 / 63 rounds and the
// exponentiations by |x| are unrolled on the host side -- so the kernel has one loop over the stream, with a
// uniform switch, and no data-dependent bound besides the one Fp inversion (fe_inv_sg, constant batches).
// Every Fp2 / Fp12 operation exists once in the code object; nothing is called, and no Fp12 value is in
// registers.  A lane takes rows lane, lane + lanes, ..: the workspace is PAIR_MAX_LANES lanes at most.
//
//   kind PAIR_IN_POINTS  cells XP, YP, QX, QY <- row i of P and Q; a row at infinity stores one and skips
//   kind PAIR_IN_ROW     slot 0 <- Fp12 row i
//   kind PAIR_IN_PAIR    slots 0, 1 <- rows 2 i, 2 i + 1 (one where there is no such row): the product tree
// and the row `out_cell` .. + 5 is stored as Fp12 row i.
#pragma once
#include <algorithm>
#include <cstring>
#include "zk_curve.hpp"
#include "zk_dispatch.hpp"
#include "zk_host.hpp"
#include "zk_pairing.hpp"
#include "zk_runtime.hpp"
#include "zk_tower.hpp"
#include "zk_pairing_prog.inc"

namespace zk {

enum { PAIR_IN_POINTS = 0, PAIR_IN_ROW = 1, PAIR_IN_PAIR = 2 };
constexpr size_t PAIR_MAX_LANES = (size_t)1 << 16;
constexpr int PAIR_BLOCK = 64;

template <class C>
__global__ void __launch_bounds__(PAIR_BLOCK) k_pair_vm(const uint32_t *__restrict__ prog, int len, int kind, int n,
                                                        int n_in, const uint64_t *__restrict__ in0,
                                                        const uint64_t *__restrict__ in1, uint64_t *__restrict__ out,
                                                        int out_cell, uint32_t *__restrict__ wsp, int lanes) {
  using F = typename C::Fp;
  using B = typename F::Base;
  constexpr int NB = B::N64;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= (size_t)lanes) return;
  const Cells<B> ws{wsp + lane, (size_t)lanes};
  for (size_t i = lane; i < (size_t)n; i += (size_t)lanes) {
    uint64_t *orow = out + i * 12 * NB;
    if (kind == PAIR_IN_POINTS) {
      const uint64_t *P = in0 + i * 2 * NB, *Q = in1 + i * 4 * NB;
      if (ref_all_ones<B>(P, 2 * NB) || ref_all_ones<B>(Q, 4 * NB)) {
        tw_one12(ws, 0);
        tw_store_row(orow, ws, 0);
        continue;
      }
#pragma unroll 1
      for (int c = 0; c < 2; c++) {
        Fe<B> x, z;
        Fe<F> v;
        ld_int(x, P + c * NB);
        fe_zero(z);
        f2_join(v, x, z);
        ws.st(ZK_PAIR_CELL_XP + c, v);
        ld_int(v, Q + c * 2 * NB);
        ws.st(ZK_PAIR_CELL_QX + c, v);
      }
    } else if (kind == PAIR_IN_ROW) {
      tw_load_row(ws, 0, in0 + i * 12 * NB);
    } else {
      tw_load_row(ws, 0, in0 + 2 * i * 12 * NB);
      if (2 * i + 1 < (size_t)n_in) tw_load_row(ws, 6, in0 + (2 * i + 1) * 12 * NB);
      else tw_one12(ws, 6);
    }
#pragma unroll 1
    for (int pc = 0; pc < len; pc++) {
      const uint32_t w = prog[pc];
      const int op = w & 255, d = (w >> 8) & 255, a = (w >> 16) & 255, b = w >> 24;
      switch (op) {
        case ZK_PAIR_OP_MUL2:
        case ZK_PAIR_OP_SQR2: {
          Fe<F> x, y, r;
          ws.ld(x, a);
          ws.ld(y, op == ZK_PAIR_OP_SQR2 ? a : b);
          fe_mul(r, x, y);
          ws.st(d, r);
          break;
        }
        case ZK_PAIR_OP_ADD2:
        case ZK_PAIR_OP_SUB2: {
          Fe<F> x, y, r;
          ws.ld(x, a);
          ws.ld(y, b);
          if (op == ZK_PAIR_OP_ADD2) fe_add(r, x, y);
          else fe_sub(r, x, y);
          ws.st(d, r);
          break;
        }
        case ZK_PAIR_OP_NEG2:
        case ZK_PAIR_OP_CONJ2:
        case ZK_PAIR_OP_COPY2: {
          Fe<F> x, r;
          ws.ld(x, a);
          if (op == ZK_PAIR_OP_NEG2) fe_neg(r, x);
          else if (op == ZK_PAIR_OP_CONJ2) f2_conj(r, x);
          else r = x;
          ws.st(d, r);
          break;
        }
        case ZK_PAIR_OP_LDC: {
          Fe<F> r;
          tw_const<B>(r, a);
          ws.st(d, r);
          break;
        }
        case ZK_PAIR_OP_INV2: {
          Fe<F> x, r;
          ws.ld(x, a);
          f2_inv(r, x);
          ws.st(d, r);
          break;
        }
        case ZK_PAIR_OP_MUL12:
        case ZK_PAIR_OP_SQR12:
        case ZK_PAIR_OP_SPMUL12:
          tw_mul12(ws, d, a, op == ZK_PAIR_OP_SQR12 ? a : b,
                   op == ZK_PAIR_OP_MUL12 ? TW_FULL : (op == ZK_PAIR_OP_SQR12 ? TW_SQUARE : TW_SPARSE));
          break;
        case ZK_PAIR_OP_FROB12:
          tw_frob12(ws, d, a);
          break;
        case ZK_PAIR_OP_CONJ12:
          tw_conj12(ws, d, a);
          break;
        case ZK_PAIR_OP_COPY12:
#pragma unroll 1
          for (int k = 0; k < 6; k++) {
            Fe<F> x;
            ws.ld(x, a + k);
            ws.st(d + k, x);
          }
          break;
        case ZK_PAIR_OP_ONE12:
          tw_one12(ws, d);
          break;
        default:
          break;
      }
    }
    tw_store_row(orow, ws, out_cell);
  }
}

template <class C>
struct PairProg;
template <>
struct PairProg<BN254_G2> {
  static constexpr const uint32_t *miller = ZK_PAIR_PROG_BN128_MILLER, *fexp = ZK_PAIR_PROG_BN128_FEXP;
  static constexpr size_t n_miller = sizeof ZK_PAIR_PROG_BN128_MILLER / 4, n_fexp = sizeof ZK_PAIR_PROG_BN128_FEXP / 4;
  static const uint64_t *one() {
    static const uint64_t v[] = ZK_BN128_FP_R64;
    return v;
  }
};
template <>
struct PairProg<BLS381_G2> {
  static constexpr const uint32_t *miller = ZK_PAIR_PROG_BLS12_381_MILLER, *fexp = ZK_PAIR_PROG_BLS12_381_FEXP;
  static constexpr size_t n_miller = sizeof ZK_PAIR_PROG_BLS12_381_MILLER / 4,
                          n_fexp = sizeof ZK_PAIR_PROG_BLS12_381_FEXP / 4;
  static const uint64_t *one() {
    static const uint64_t v[] = ZK_BLS12_381_FP_R64;
    return v;
  }
};
// the product tree's stream: slot 2 <- slot 0 times slot 1
constexpr uint32_t PAIR_PROG_MUL[] = {ZK_PAIR_OP_MUL12 | 12u << 8 | 0u << 16 | 6u << 24};

inline size_t pair_lanes(size_t n) {
  return (std::min(std::max(n, (size_t)1), PAIR_MAX_LANES) + PAIR_BLOCK - 1) / PAIR_BLOCK * PAIR_BLOCK;
}

template <class C>
struct PairCall {
  using B = typename C::Fp::Base;
  static constexpr int NB = B::N64;
  static constexpr size_t ROW = 12 * NB;
  Device &dev;
  uint32_t *ws = nullptr, *d_miller = nullptr, *d_fexp = nullptr, *d_both = nullptr, *d_mul = nullptr;
  size_t lanes = 0;
  explicit PairCall(Device &d) : dev(d) {}
  static size_t ws_bytes(size_t n) { return pair_lanes(n) * ZK_PAIR_NCELL * 2 * B::N * 4; }
  static size_t prog_bytes() { return (2 * (PairProg<C>::n_miller + PairProg<C>::n_fexp) + 1) * 4 + 5 * 256; }
  void setup(size_t n) {
    using PP = PairProg<C>;
    lanes = pair_lanes(n);
    ws = dev.arena.take<uint32_t>(lanes * ZK_PAIR_NCELL * 2 * B::N);
    d_both = dev.arena.take<uint32_t>(PP::n_miller + PP::n_fexp);
    d_miller = dev.arena.take<uint32_t>(PP::n_miller);
    d_fexp = dev.arena.take<uint32_t>(PP::n_fexp);
    d_mul = dev.arena.take<uint32_t>(1);
    ZK_CHECK(hipMemcpyAsync(d_both, PP::miller, PP::n_miller * 4, hipMemcpyHostToDevice, dev.stream));
    ZK_CHECK(hipMemcpyAsync(d_both + PP::n_miller, PP::fexp, PP::n_fexp * 4, hipMemcpyHostToDevice, dev.stream));
    ZK_CHECK(hipMemcpyAsync(d_miller, PP::miller, PP::n_miller * 4, hipMemcpyHostToDevice, dev.stream));
    ZK_CHECK(hipMemcpyAsync(d_fexp, PP::fexp, PP::n_fexp * 4, hipMemcpyHostToDevice, dev.stream));
    ZK_CHECK(hipMemcpyAsync(d_mul, PAIR_PROG_MUL, 4, hipMemcpyHostToDevice, dev.stream));
  }
  void run(const uint32_t *prog, size_t len, int kind, size_t n, size_t n_in, const uint64_t *in0, const uint64_t *in1,
           uint64_t *out, int out_cell) {
    const size_t use = pair_lanes(n);  // <= lanes: the workspace was sized for the call's largest launch
    hipLaunchKernelGGL(k_pair_vm<C>, dim3((unsigned)(use / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, dev.stream, prog, (int)len,
                       kind, (int)n, (int)n_in, in0, in1, out, out_cell, ws, (int)use);
    ZK_CHECK(hipGetLastError());
  }
};

template <class C>
void pairing_rows_t(Device &dev, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io) {
  using PC = PairCall<C>;
  using PP = PairProg<C>;
  constexpr int NB = PC::NB;
  if (n <= 0) return;
  const size_t N = (size_t)n;
  dev.arena.reserve(PC::ws_bytes(N) + PC::prog_bytes() + (host_io ? N * (6 + 12) * NB * 8 + 1024 : 0) + (1 << 16));
  dev.arena.reset();
  StagedIO io(dev, host_io, P, N * 2 * NB, tgt, N * PC::ROW);
  const uint64_t *d_q = Q;
  if (host_io) {
    uint64_t *dq = dev.arena.take<uint64_t>(N * 4 * NB);
    ZK_CHECK(hipMemcpyAsync(dq, Q, N * 4 * NB * 8, hipMemcpyHostToDevice, dev.stream));
    d_q = dq;
  }
  PC call(dev);
  call.setup(N);
  call.run(call.d_both, PP::n_miller + PP::n_fexp, PAIR_IN_POINTS, N, N, io.in, d_q, io.out, 0);
  io.finish();
}

template <class C>
void pairing_final_expo_t(Device &dev, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  using PC = PairCall<C>;
  using PP = PairProg<C>;
  if (n <= 0) return;
  const size_t N = (size_t)n;
  dev.arena.reserve(PC::ws_bytes(N) + PC::prog_bytes() + (host_io ? 2 * N * PC::ROW * 8 + 1024 : 0) + (1 << 16));
  dev.arena.reset();
  StagedIO io(dev, host_io, src, N * PC::ROW, tgt, N * PC::ROW);
  PC call(dev);
  call.setup(N);
  call.run(call.d_fexp, PP::n_fexp, PAIR_IN_ROW, N, N, io.in, nullptr, io.out, 0);
  io.finish();
}

template <class C>
void pairing_product_t(Device &dev, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io) {
  using PC = PairCall<C>;
  using PP = PairProg<C>;
  constexpr int NB = PC::NB;
  const size_t N = (size_t)std::max(n, 0);
  if (N == 0) {  // the empty product: Montgomery one
    uint64_t one[PC::ROW] = {};
    memcpy(one, PP::one(), NB * 8);
    if (host_io) memcpy(tgt, one, sizeof one);
    else ZK_CHECK(hipMemcpy(tgt, one, sizeof one, hipMemcpyHostToDevice));
    return;
  }
  dev.arena.reserve(PC::ws_bytes(N) + PC::prog_bytes() + (host_io ? N * 6 * NB * 8 + PC::ROW * 8 + 1024 : 0) +
                    2 * N * PC::ROW * 8 + (1 << 16));
  dev.arena.reset();
  StagedIO io(dev, host_io, P, N * 2 * NB, tgt, PC::ROW);
  const uint64_t *d_q = Q;
  if (host_io) {
    uint64_t *dq = dev.arena.take<uint64_t>(N * 4 * NB);
    ZK_CHECK(hipMemcpyAsync(dq, Q, N * 4 * NB * 8, hipMemcpyHostToDevice, dev.stream));
    d_q = dq;
  }
  uint64_t *a = dev.arena.take<uint64_t>(N * PC::ROW), *b = dev.arena.take<uint64_t>(N * PC::ROW);
  PC call(dev);
  call.setup(N);
  call.run(call.d_miller, PP::n_miller, PAIR_IN_POINTS, N, N, io.in, d_q, a, 0);
  for (size_t m = N; m > 1; m = (m + 1) / 2) {  // the tree product of the Miller values
    call.run(call.d_mul, 1, PAIR_IN_PAIR, (m + 1) / 2, m, a, nullptr, b, 12);
    std::swap(a, b);
  }
  call.run(call.d_fexp, PP::n_fexp, PAIR_IN_ROW, 1, 1, a, nullptr, io.out, 0);
  io.finish();
}

#define ZK_PAIRING_INSTANCES(KW, C)                                                                                 \
  KW template void pairing_rows_t<C>(Device &, int, const uint64_t *, const uint64_t *, uint64_t *, bool);          \
  KW template void pairing_product_t<C>(Device &, int, const uint64_t *, const uint64_t *, uint64_t *, bool);       \
  KW template void pairing_final_expo_t<C>(Device &, int, const uint64_t *, uint64_t *, bool);

}  // namespace zk
