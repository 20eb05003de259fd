/* Run-time K -> compile-time KMAX: the kernels keep per-cluster values in register arrays sized by a template
 * parameter, so every launch site picks an instance from the number of clusters.  A ladder is the list of sizes a site
 * has instances for; kdispatch calls f(std::integral_constant<int, KM>()) with the first rung KM >= K, and with the
 * last rung for every K above it (the callers' own caps keep such K away, or the last rung is a K-generic kernel).
 *
 * A generic callable is instantiated for EVERY rung of the ladder it is given: a site takes the ladder that lists
 * exactly its instances, or kernels nobody launches get compiled.  Host only, no HIP in here (tests/test_kdispatch.py
 * compiles it with the host compiler). */
#ifndef ISG_KDISPATCH_H
#define ISG_KDISPATCH_H
#include <type_traits>

template <int... RUNGS>
struct KLadder {};

template <class F, int R0, int... REST>
static inline void kdispatch(KLadder<R0, REST...>, int K, F &&f)
{
	if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, R0>());
	else if (K <= R0) f(std::integral_constant<int, R0>());
	else kdispatch(KLadder<REST...>(), K, f);
}

/* ploidy 2 */
using KL_ZQ = KLadder<2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 64>; /* k_zq, k_zexpect, k_zq_probe, k_zq_at: exact sizes for small K, rounded up above; 64 = the K-generic wide form */
using KL_ZQ_COOP = KLadder<2, 3, 4, 5, 6, 8, 12, 16, 24, 32>; /* k_zq_coop: the register-resident cap */
using KL_ZQ_8 = KLadder<2, 3, 4, 5, 6, 8>;                  /* k_zq_pipe, k_zq_spec, the block resolver's k_zq_at: paths taken for K <= 8 only */
using KL_ZQ_EXACT = KLadder<2, 3, 4, 5, 6, 7, 8>;           /* k_zq_block(s): K == KMAX is a compile-time constant there (K = 1 runs in the 2 instance) */
/* ploidy 4 */
using KL_P4 = KLadder<2, 4, 6, 8, 12, 16, 24, 32>;         /* k4_zq, k4_zq_coop, k4_zexpect*, k4_zq_probe */
using KL_P4_BLOCK = KLadder<2, 4, 6, 8, 12, 16>;            /* k4_zq_block and its k4_zq: the block resolver stops at K = 16 */
using KL_P4_GENO = KLadder<4, 8, 12, 16, 32>;               /* k4_geno: whole float4 rows of the admixture vector */

#endif
