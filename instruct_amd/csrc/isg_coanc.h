/* The posterior co-ancestry accumulation (isg_coanc_hip.inc, k_coanc_syrk): how the N x N accumulator is cut into tiles, which
 * workgroup owns which tile pair, how the snapshot history is padded, and which element of an operand or of the result a lane of the
 * f64 matrix instruction holds.  Plain values and integer arithmetic only, no HIP in here: the kernel includes it, and
 * tests/test_coanc_layout.py compiles it with the host compiler (tests/emul/coanc_emul.cpp). */
#ifndef ISG_COANC_H
#define ISG_COANC_H
#include <stddef.h>

#define ISG_COANC_TILE 64                                  /* a workgroup's tile of the accumulator is TILE x TILE ... */
#define ISG_COANC_SUB 16                                   /* ... cut into SUB x SUB results of one matrix instruction */
#define ISG_COANC_KSTEP 4                                  /* inner columns one matrix instruction consumes */
#define ISG_COANC_WAVES (ISG_COANC_TILE / ISG_COANC_SUB)   /* wave w: sub-row w of the tile ... */
#define ISG_COANC_NSUB (ISG_COANC_TILE / ISG_COANC_SUB)    /* ... all NSUB sub-columns: NSUB independent accumulators */
#define ISG_COANC_BLOCK (64 * ISG_COANC_WAVES)
#define ISG_COANC_BATCH 8                                  /* snapshots per flush when the caller passes 0 (DESIGN.md "Posterior co-ancestry") */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISG_COANC_HD __host__ __device__ __forceinline__
#else
#define ISG_COANC_HD static inline
#endif

/* padding: clusters to a whole number of instruction steps, individuals to whole tiles; the padding holds zeros */
ISG_COANC_HD int isg_coanc_kp(int K) { return (K + ISG_COANC_KSTEP - 1) / ISG_COANC_KSTEP * ISG_COANC_KSTEP; }
ISG_COANC_HD int isg_coanc_np(int N) { return (N + ISG_COANC_TILE - 1) / ISG_COANC_TILE * ISG_COANC_TILE; }
ISG_COANC_HD int isg_coanc_tiles(int N) { return isg_coanc_np(N) / ISG_COANC_TILE; }
/* workgroups of a flush: the tile pairs (ti, tj) with tj <= ti */
ISG_COANC_HD long isg_coanc_groups(int N) { const long T = isg_coanc_tiles(N); return T * (T + 1) / 2; }
/* history: [batch][Np][Kp] doubles; element (snapshot t, individual i, cluster k) */
ISG_COANC_HD size_t isg_coanc_hist_stride(int N, int K) { return (size_t)isg_coanc_np(N) * isg_coanc_kp(K); }
ISG_COANC_HD size_t isg_coanc_hist_index(int t, int i, int k, int Np, int Kp) { return ((size_t)t * Np + i) * Kp + k; }

/* workgroup w = ti (ti + 1) / 2 + tj  ->  (ti, tj), tj <= ti: the largest ti with ti (ti + 1) / 2 <= w by bisection (ti < 2^16) */
ISG_COANC_HD void isg_coanc_decode(unsigned w, int *ti, int *tj)
{
	unsigned lo = 0, hi = 1u << 16;
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if ((unsigned long long)mid * (mid + 1) / 2 <= w) lo = mid; else hi = mid;
	}
	*ti = (int)lo;
	*tj = (int)(w - lo * (lo + 1) / 2);
}

/* v_mfma_f64_16x16x4_f64, D = A B + C with A 16 x 4, B 4 x 16: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15], one double
 * each, and holds the four results D[(l >> 4) + 4 reg][l & 15], reg 0 .. 3 (not the f32 forms' 4 (l >> 4) + reg) */
ISG_COANC_HD int isg_coanc_ab_idx(int lane) { return lane & 15; } /* A: row, B: column */
ISG_COANC_HD int isg_coanc_ab_k(int lane) { return lane >> 4; }
ISG_COANC_HD int isg_coanc_cd_col(int lane) { return lane & 15; }
ISG_COANC_HD int isg_coanc_cd_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }

/* what wave `wave`, lane `lane` of the workgroup of tile pair (ti, tj) touches:
 * its A operand of inner step (t, k0) is hist[t][isg_coanc_a_row][k0 + isg_coanc_ab_k], its B operand of sub-column s
 * hist[t][isg_coanc_b_row][k0 + isg_coanc_ab_k] (B = Q^T: a column of B is a row of Q, so both are plain loads), and register reg of
 * its accumulator s is Acc[isg_coanc_c_row][isg_coanc_c_col] */
ISG_COANC_HD int isg_coanc_a_row(int ti, int wave, int lane) { return ti * ISG_COANC_TILE + wave * ISG_COANC_SUB + isg_coanc_ab_idx(lane); }
ISG_COANC_HD int isg_coanc_b_row(int tj, int s, int lane) { return tj * ISG_COANC_TILE + s * ISG_COANC_SUB + isg_coanc_ab_idx(lane); }
ISG_COANC_HD int isg_coanc_c_row(int ti, int wave, int lane, int reg) { return ti * ISG_COANC_TILE + wave * ISG_COANC_SUB + isg_coanc_cd_row(lane, reg); }
ISG_COANC_HD int isg_coanc_c_col(int tj, int s, int lane) { return tj * ISG_COANC_TILE + s * ISG_COANC_SUB + isg_coanc_cd_col(lane); }

/* bytes isg_coanc_begin asks the device for */
ISG_COANC_HD size_t isg_coanc_bytes(int N, int K, int batch) { return sizeof(double) * ((size_t)N * N + (size_t)batch * isg_coanc_hist_stride(N, K)); }

#endif
