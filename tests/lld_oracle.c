/* Test oracle of the two-piece local-alignment contract (include/ksw2_amd.h, ksw2amd_lld_batch): a plain scalar Smith-Waterman over the
 * full matrix with two independent pairs of Gotoh gap states.  H(i,j) = max(0, H(i-1,j-1) + mat[t_i * m + q_j], E, F, E2, F2),
 * E / F = max(H - (gapo + gape), E / F - gape), E2 / F2 = max(H - (gapo2 + gape2), E2 / F2 - gape2): a gap of length l costs
 * min(gapo + l * gape, gapo2 + l * gape2).  The gap states are NOT clamped here.  The best cell is the largest H, then the smallest te,
 * then the smallest qe; a best score of 0 gives (-1, -1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

int lld_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2,
               int *qe, int *te)
{
	const int64_t NEG = -((int64_t)1 << 40);
	int64_t *H, *E, *E2, best = 0;
	int i, j, bq = -1, bt = -1;
	*qe = *te = -1;
	if (qlen <= 0 || tlen <= 0) return 0;
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	E2 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	for (j = 0; j <= qlen; ++j) { H[j] = 0; E[j] = E2[j] = NEG; }
	for (i = 0; i < tlen; ++i) {                                      /* rows = target: row order is te order */
		int64_t diag = 0, F = NEG, F2 = NEG, hleft = 0;
		for (j = 0; j < qlen; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e, f, e2, f2;
			e = E[j + 1] - gape; if (up - gapo - gape > e) e = up - gapo - gape;
			f = F - gape; if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			e2 = E2[j + 1] - gape2; if (up - gapo2 - gape2 > e2) e2 = up - gapo2 - gape2;
			f2 = F2 - gape2; if (hleft - gapo2 - gape2 > f2) f2 = hleft - gapo2 - gape2;
			h = diag + mat[target[i] * m + query[j]];
			if (e > h) h = e;
			if (f > h) h = f;
			if (e2 > h) h = e2;
			if (f2 > h) h = f2;
			if (h < 0) h = 0;
			E[j + 1] = e; F = f; E2[j + 1] = e2; F2 = f2;
			diag = up; H[j + 1] = h; hleft = h;
			if (h > best) { best = h; bt = i; bq = j; }     /* strict: first in (te, qe) order among equals */
		}
	}
	free(H); free(E); free(E2);
	*qe = bq; *te = bt;
	return (int)best;
}

/* n pairs from one arena: out[3 i ..] = score, qe, te */
void lld_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                      int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) {
		int qe, te;
		out[3 * i] = lld_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, gapo2, gape2, &qe, &te);
		out[3 * i + 1] = qe; out[3 * i + 2] = te;
	}
}
