/* Test oracle of ksw2amd_sgd_batch / ksw2amd_sgd_align_batch's coordinates (include/ksw2_amd.h): plain scalar int64
 * with -infinity boundaries, no clamp, no bias, the two-piece cost cost(l) = min(gapo + l * gape, gapo2 + l * gape2) with the pieces as given.
 *   forward: H(t, -1) = 0, H(-1, j) = -cost(j + 1), H = max(diag + s, E, F, E2, F2) with ksw_extd's four gap states;
 *            score = the largest H(t, qlen - 1), te = the smallest such t;
 *   start:   G(x) = the GLOBAL score of the whole query against target[x..te] (boundaries -cost(k) on both sides), G(te + 1) = -cost(qlen);
 *            tb = the largest x in [0, te + 1] with G(x) == score.  One anchored matrix gives every G(x): the global alignment of
 *            reverse(query) against reverse(target[0..te]) holds G(te - i) in row i of its last column.
 * out[6 i ..] = score, qb, qe, tb, te, found (1: some x reached the score -- the contract says always).
 * qlen <= 0: (0, -1, -1, -1, -1, 1); tlen <= 0: (-cost(qlen), 0, qlen - 1, 0, -1, 1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

#define NEG (-((int64_t)1 << 50))

typedef struct { int64_t o, e, o2, e2; } sgd_cost_t;

static int64_t sgd_cost(const sgd_cost_t *c, int64_t l)
{
	const int64_t a = c->o + l * c->e, b = c->o2 + l * c->e2;
	return a < b ? a : b;
}

/* one row of the matrix: H[], E[], E2[] hold row i - 1 on entry and row i on return; left = H(i, -1), diag0 = H(i - 1, -1) */
static void sgd_row(int qlen, const uint8_t *query, int qrev, int tc, int m, const int8_t *mat, const sgd_cost_t *c, int64_t left, int64_t diag0,
                    int64_t *H, int64_t *E, int64_t *E2)
{
	int64_t diag = diag0, F = NEG, F2 = NEG, hleft = left;
	int j;
	for (j = 0; j < qlen; ++j) {
		const int64_t up = H[j + 1];
		const int qc = query[qrev ? qlen - 1 - j : j];
		int64_t h, e = E[j + 1] - c->e, e2 = E2[j + 1] - c->e2, f = F - c->e, f2 = F2 - c->e2;
		if (up - c->o - c->e > e) e = up - c->o - c->e;
		if (up - c->o2 - c->e2 > e2) e2 = up - c->o2 - c->e2;
		if (hleft - c->o - c->e > f) f = hleft - c->o - c->e;
		if (hleft - c->o2 - c->e2 > f2) f2 = hleft - c->o2 - c->e2;
		h = diag + mat[tc * m + qc];
		if (e > h) h = e;
		if (f > h) h = f;
		if (e2 > h) h = e2;
		if (f2 > h) h = f2;
		E[j + 1] = e; E2[j + 1] = e2; F = f; F2 = f2; diag = up; H[j + 1] = h; hleft = h;
	}
}

static void sgd_top(int qlen, const sgd_cost_t *c, int64_t *H, int64_t *E, int64_t *E2)
{
	int j;
	H[0] = 0; E[0] = E2[0] = NEG;
	for (j = 1; j <= qlen; ++j) { H[j] = -sgd_cost(c, j); E[j] = E2[j] = NEG; }
}

static int64_t sgd_forward(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, const sgd_cost_t *c, int *te)
{
	int64_t *H = (int64_t*)malloc(sizeof(int64_t) * 3 * (size_t)(qlen + 1)), *E = H + qlen + 1, *E2 = E + qlen + 1, best = NEG;
	int i;
	sgd_top(qlen, c, H, E, E2);
	for (i = 0; i < tlen; ++i) {
		sgd_row(qlen, query, 0, target[i], m, mat, c, 0, 0, H, E, E2);      /* column -1: H = 0 in every row */
		if (H[qlen] > best) { best = H[qlen]; *te = i; }
	}
	free(H);
	return best;
}

/* the largest x in [0, te + 1] with G(x) == score, -1 if there is none */
static int sgd_start(int qlen, const uint8_t *query, int te, const uint8_t *target, int m, const int8_t *mat, const sgd_cost_t *c, int64_t score)
{
	int64_t *H = (int64_t*)malloc(sizeof(int64_t) * 3 * (size_t)(qlen + 1)), *E = H + qlen + 1, *E2 = E + qlen + 1;
	int i, tb = -1;
	sgd_top(qlen, c, H, E, E2);
	if (H[qlen] == score) tb = te + 1;                                 /* the empty interval: it wins its ties */
	for (i = 0; i <= te && tb < 0; ++i) {                              /* row i = target[te - i], column j = query[qlen - 1 - j] */
		const int64_t left = -sgd_cost(c, i + 1), diag0 = H[0];
		H[0] = left;
		sgd_row(qlen, query, 1, target[te - i], m, mat, c, left, diag0, H, E, E2);
		if (H[qlen] == score) tb = te - i;                             /* the first row that reaches it: the shortest interval */
	}
	free(H);
	return tb;
}

void sgd_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                      int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int32_t *out)
{
	sgd_cost_t c;
	int i;
	c.o = gapo; c.e = gape; c.o2 = gapo2; c.e2 = gape2;
	for (i = 0; i < n; ++i) {
		int32_t *o = out + 6 * i;
		const int ql = qlen[i], tl = tlen[i];
		int te = -1, tb;
		int64_t s;
		if (ql <= 0) { o[0] = 0; o[1] = o[2] = o[3] = o[4] = -1; o[5] = 1; continue; }
		if (tl <= 0) { o[0] = (int32_t)-sgd_cost(&c, ql); o[1] = 0; o[2] = ql - 1; o[3] = 0; o[4] = -1; o[5] = 1; continue; }
		s = sgd_forward(ql, base + qoff[i], tl, base + toff[i], m, mat, &c, &te);
		tb = sgd_start(ql, base + qoff[i], te, base + toff[i], m, mat, &c, s);
		o[0] = (int32_t)s; o[1] = 0; o[2] = ql - 1; o[3] = tb; o[4] = te; o[5] = tb >= 0;
	}
}
