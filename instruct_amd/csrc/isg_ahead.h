/* What the replay iteration has enqueued AHEAD of the host look it was waiting for (isg_iteration's launch-ahead mode, DESIGN.md
 * "Replay iteration: looks and launch-ahead"), and what makes each of those results stale.  A result is a device-side by-product of a
 * kernel that ran earlier than its sweep would have launched it; a bit says it may be used in place of launching the kernel again.
 * Plain values only, no HIP in here: isg_hip.hip and its includes call it, and tests/test_ahead_state.py compiles it with the host
 * compiler.
 *
 *   item          kernels                                      reads                      enqueued behind the look of
 *   AH_FREQF      k_freqf + k_lltab(_int)  (refresh_freqf)     freq                       update_P
 *   AH_EXPECT     update_ZQ's base-free prologue: the memsets, qq, freqf, alpha           update_G
 *                 the qq save, k_zexpect, k_wk_bpred, k_wk_centers
 *   AH_LKH        cal_lkh's likelihood sweep                   Z, qq, generations, tables update_ZQ
 *   AH_LKH_TOTAL  k_lkh_total                                  indvlkh (AH_LKH's output)  update_alpha
 *   AH_COUNTS     the next update_P's k_count (+ k_pd_gather,  Z                          update_alpha
 *                 k_pd_scan when update_P runs on the device)
 *
 * Only AH_COUNTS may outlive the iteration that made it.
 */
#ifndef ISG_AHEAD_H
#define ISG_AHEAD_H

enum {
	AH_FREQF = 1u << 0,
	AH_EXPECT = 1u << 1,
	AH_LKH = 1u << 2,
	AH_LKH_TOTAL = 1u << 3,
	AH_COUNTS = 1u << 4,
	AH_ALL = (1u << 5) - 1u
};
/* the host looks of the replay iteration: each has a slot in the context's pinned mailbox and an event recorded behind its copies */
enum { AH_LOOK_P, AH_LOOK_G, AH_LOOK_ZQ, AH_LOOK_ALPHA, AH_NLOOKS };

struct AheadState {
	unsigned have;    /* AH_* results that exist on the device and are current */
	unsigned pending; /* bit l: look l's event is recorded and nobody has waited for it yet */
};

static inline void ahead_init(AheadState *s) { s->have = 0u; s->pending = 0u; }
static inline bool ahead_has(const AheadState *s, unsigned item) { return (s->have & item) == item; }
/* (the total is a function of the sweep's output: it goes whenever the sweep goes) */
static inline void ahead_clear(AheadState *s, unsigned items)
{
	if (items & AH_LKH) items |= AH_LKH_TOTAL;
	s->have &= ~items;
}
/* the kernels of `item` have been enqueued; the total only counts on top of a current sweep */
static inline void ahead_set(AheadState *s, unsigned item)
{
	if ((item & AH_LKH_TOTAL) && !((s->have | item) & AH_LKH)) item &= ~(unsigned)AH_LKH_TOTAL;
	s->have |= item & AH_ALL;
}
/* the consumer's question: true (and the item is used up) if its kernels need not be launched */
static inline bool ahead_take(AheadState *s, unsigned item)
{
	const bool had = ahead_has(s, item);
	ahead_clear(s, item);
	return had;
}

/* ---- invalidation: what a write makes stale ---- */
static inline void ahead_wrote_z(AheadState *s) { ahead_clear(s, AH_COUNTS | AH_LKH); }            /* update_ZQ, update_Z, chain_init, set_z */
static inline void ahead_wrote_freq(AheadState *s) { ahead_clear(s, AH_FREQF | AH_EXPECT | AH_LKH); } /* update_P's draws, set_freq */
static inline void ahead_wrote_qq(AheadState *s) { ahead_clear(s, AH_EXPECT | AH_LKH); }           /* update_ZQ, set_qq */
static inline void ahead_wrote_gen(AheadState *s) { ahead_clear(s, AH_LKH); }                      /* update_G, set_generation */
static inline void ahead_wrote_alpha(AheadState *s) { ahead_clear(s, AH_EXPECT); }                 /* update_alpha, set_alpha */
static inline void ahead_chain_init(AheadState *s) { ahead_clear(s, AH_ALL); }
/* the end of isg_iteration: whatever was not consumed inside it is dropped, the next update_P's counts stay */
static inline void ahead_end_iteration(AheadState *s) { ahead_clear(s, AH_ALL & ~(unsigned)AH_COUNTS); }

/* ---- looks ---- */
static inline void ahead_look_recorded(AheadState *s, int look) { s->pending |= 1u << look; }
static inline void ahead_look_waited(AheadState *s, int look) { s->pending &= ~(1u << look); }
/* the looks the caller has to wait for before it reads or changes host state; none are pending afterwards (a second call returns 0) */
static inline unsigned ahead_settle(AheadState *s)
{
	const unsigned m = s->pending;
	s->pending = 0u;
	return m;
}

#endif
