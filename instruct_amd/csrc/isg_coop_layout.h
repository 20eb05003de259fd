/* How the cooperative update_ZQ kernels (isg_coop_hip.inc, k4_zq_coop) lay an individual's counts out in the tagged
 * 8-byte granules they exchange.  Plain values and integer arithmetic only, no HIP in here: the kernels include it,
 * and tests/test_coop_layout.py compiles it with the host compiler. */
#ifndef ISG_COOP_LAYOUT_H
#define ISG_COOP_LAYOUT_H

#define ISG_COOP_RING 4
#define ISG_COOP_GMAX 128
#define ISG_COOP_WMAX 11

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISG_COOP_HD __host__ __device__ __forceinline__
#else
#define ISG_COOP_HD static inline
#endif

struct CoopLayout {
	bool wmode; /* few workgroups: every WAVE publishes granules of its own and one polling round covers them all */
	int pack;   /* counts per exchanged word ... */
	int bits;   /* ... of this many bits each: 3 x 16, or 4 x 12 */
	int W;      /* words per publisher */
	int ngran;  /* granules of one individual: publishers x W */
};

/* G workgroups of BLOCK lanes, K clusters, Lp loci of `copies` allele copies each (one locus per lane and pass) */
ISG_COOP_HD CoopLayout coop_layout(int G, int BLOCK, int K, int Lp, int copies)
{
	CoopLayout l;
	l.wmode = (G * (BLOCK / 64) * ((K + 2) / 3) <= BLOCK); /* one polling round covers a granule per wave */
	/* counts per exchanged word: 3 x 16 bits, or 4 x 12 bits when a workgroup's count of one bucket stays below 4096 */
	const int npass = (Lp + G * BLOCK - 1) / (G * BLOCK);
	l.pack = (!l.wmode && copies * BLOCK * npass < 4096) ? 4 : 3;
	l.bits = (l.pack == 4) ? 12 : 16;
	l.W = (K + l.pack - 1) / l.pack;
	l.ngran = l.wmode ? G * (BLOCK / 64) * l.W : G * l.W;
	return l;
}

#endif
