/* Test oracle of ksw2amd_sg_align_batch's coordinates (include/ksw2_amd.h): plain scalar int64 with -infinity boundaries, no clamp, no bias.
 *   forward: the semi-global formula of tests/sg_oracle.c restated -- score = the largest H(t, qlen - 1), te = the smallest such t;
 *   start:   G(x) = the GLOBAL score of the whole query against target[x..te] (boundaries -(gapo + k * gape) on both sides), G(te + 1) =
 *            -(gapo + qlen * gape); tb = the largest x in [0, te + 1] with G(x) == score.  One anchored matrix gives every G(x): the global
 *            alignment of reverse(query) against reverse(target[0..te]) holds G(te - i) in row i of its last column.
 * out[6 i ..] = score, qb, qe, tb, te, found (1: some x reached the score -- the contract says always).
 * qlen <= 0: (0, -1, -1, -1, -1, 1); tlen <= 0: (-(gapo + qlen * gape), 0, qlen - 1, 0, -1, 1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

#define NEG (-((int64_t)1 << 50))

static int64_t sga_forward(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int *te)
{
	int64_t *H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1)), *E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1)), best = NEG;
	int i, j;
	H[0] = 0; E[0] = NEG;
	for (j = 1; j <= qlen; ++j) { H[j] = -((int64_t)gapo + (int64_t)j * gape); E[j] = NEG; }
	for (i = 0; i < tlen; ++i) {
		int64_t diag = 0, F = NEG, hleft = 0;                          /* column -1: H = 0 in every row */
		for (j = 0; j < qlen; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e = E[j + 1] - gape, f = F - gape;
			if (up - gapo - gape > e) e = up - gapo - gape;
			if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			h = diag + mat[target[i] * m + query[j]];
			if (e > h) h = e;
			if (f > h) h = f;
			E[j + 1] = e; F = f; diag = up; H[j + 1] = h; hleft = h;
		}
		if (H[qlen] > best) { best = H[qlen]; *te = i; }
	}
	free(H); free(E);
	return best;
}

/* the largest x in [0, te + 1] with G(x) == score, -1 if there is none */
static int sga_start(int qlen, const uint8_t *query, int te, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int64_t score)
{
	int64_t *H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1)), *E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	int i, j, tb = -1;
	H[0] = 0; E[0] = NEG;
	for (j = 1; j <= qlen; ++j) { H[j] = -((int64_t)gapo + (int64_t)j * gape); E[j] = NEG; }
	if (H[qlen] == score) tb = te + 1;                                 /* the empty interval: it wins its ties */
	for (i = 0; i <= te && tb < 0; ++i) {                              /* row i = target[te - i], column j = query[qlen - 1 - j] */
		const int64_t left = -((int64_t)gapo + (int64_t)(i + 1) * gape);
		int64_t diag = H[0], F = NEG, hleft = left;
		H[0] = left;
		for (j = 0; j < qlen; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e = E[j + 1] - gape, f = F - gape;
			if (up - gapo - gape > e) e = up - gapo - gape;
			if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			h = diag + mat[target[te - i] * m + query[qlen - 1 - j]];
			if (e > h) h = e;
			if (f > h) h = f;
			E[j + 1] = e; F = f; diag = up; H[j + 1] = h; hleft = h;
		}
		if (H[qlen] == score) tb = te - i;                             /* the first row that reaches it: the shortest interval */
	}
	free(H); free(E);
	return tb;
}

void sga_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                      int m, const int8_t *mat, int gapo, int gape, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) {
		int32_t *o = out + 6 * i;
		const int ql = qlen[i], tl = tlen[i];
		int te = -1, tb;
		int64_t s;
		if (ql <= 0) { o[0] = 0; o[1] = o[2] = o[3] = o[4] = -1; o[5] = 1; continue; }
		if (tl <= 0) { o[0] = -(gapo + ql * gape); o[1] = 0; o[2] = ql - 1; o[3] = 0; o[4] = -1; o[5] = 1; continue; }
		s = sga_forward(ql, base + qoff[i], tl, base + toff[i], m, mat, gapo, gape, &te);
		tb = sga_start(ql, base + qoff[i], te, base + toff[i], m, mat, gapo, gape, s);
		o[0] = (int32_t)s; o[1] = 0; o[2] = ql - 1; o[3] = tb; o[4] = te; o[5] = tb >= 0;
	}
}
