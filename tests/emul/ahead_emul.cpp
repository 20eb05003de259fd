/* Drives instruct_amd/csrc/isg_ahead.h on the host: one line "name have pending" per scenario (tests/test_ahead_state.py holds the
 * expected values).  Bits are printed as numbers; "BITS" gives their values first. */
#include <stdio.h>
#include "../../instruct_amd/csrc/isg_ahead.h"

typedef void (*Rule)(AheadState *);
static void show(const char *name, const AheadState &s) { printf("%s %u %u\n", name, s.have, s.pending); }

int main()
{
	printf("BITS %u %u %u %u %u %u %d\n", (unsigned)AH_FREQF, (unsigned)AH_EXPECT, (unsigned)AH_LKH, (unsigned)AH_LKH_TOTAL, (unsigned)AH_COUNTS, (unsigned)AH_ALL, (int)AH_NLOOKS);
	const struct { const char *name; Rule rule; } rules[] = {
		{"wrote_z", ahead_wrote_z}, {"wrote_freq", ahead_wrote_freq}, {"wrote_qq", ahead_wrote_qq}, {"wrote_gen", ahead_wrote_gen},
		{"wrote_alpha", ahead_wrote_alpha}, {"chain_init", ahead_chain_init}, {"end_iteration", ahead_end_iteration},
	};
	char name[64];
	for (const auto &r : rules) {
		AheadState s;
		ahead_init(&s);
		ahead_set(&s, AH_ALL);
		ahead_look_recorded(&s, AH_LOOK_ALPHA); /* a rule never touches the looks */
		r.rule(&s);
		snprintf(name, sizeof(name), "all_%s", r.name);
		show(name, s);
		/* every single item on its own: a rule clears it or leaves it, and sets nothing */
		for (unsigned b = 1; b <= AH_COUNTS; b <<= 1) {
			ahead_init(&s);
			ahead_set(&s, b == AH_LKH_TOTAL ? (unsigned)(AH_LKH | AH_LKH_TOTAL) : b);
			r.rule(&s);
			snprintf(name, sizeof(name), "one_%u_%s", b, r.name);
			show(name, s);
		}
		ahead_init(&s);
		r.rule(&s);
		snprintf(name, sizeof(name), "none_%s", r.name);
		show(name, s);
	}
	AheadState s;
	ahead_init(&s);
	show("init", s);
	ahead_set(&s, AH_LKH_TOTAL); /* no sweep to be the total of */
	show("total_without_sweep", s);
	ahead_set(&s, AH_LKH);
	ahead_set(&s, AH_LKH_TOTAL);
	show("sweep_then_total", s);
	printf("take_total %d\n", ahead_take(&s, AH_LKH_TOTAL) ? 1 : 0);
	show("after_take_total", s);
	ahead_set(&s, AH_LKH_TOTAL);
	printf("take_sweep %d\n", ahead_take(&s, AH_LKH) ? 1 : 0); /* the total goes with it */
	show("after_take_sweep", s);
	printf("take_again %d\n", ahead_take(&s, AH_LKH) ? 1 : 0);
	ahead_set(&s, AH_COUNTS | AH_FREQF);
	printf("has_counts %d has_both %d has_expect %d\n", ahead_has(&s, AH_COUNTS) ? 1 : 0, ahead_has(&s, AH_COUNTS | AH_FREQF) ? 1 : 0, ahead_has(&s, AH_EXPECT) ? 1 : 0);
	ahead_set(&s, 1u << 9); /* not an item */
	show("unknown_bit", s);
	/* looks */
	ahead_look_recorded(&s, AH_LOOK_P);
	ahead_look_recorded(&s, AH_LOOK_ZQ);
	show("two_looks", s);
	ahead_look_waited(&s, AH_LOOK_P);
	show("one_waited", s);
	ahead_look_recorded(&s, AH_LOOK_G);
	printf("settle %u\n", ahead_settle(&s));
	show("settled", s);
	printf("settle_again %u\n", ahead_settle(&s));
	show("settled_again", s);
	return 0;
}
