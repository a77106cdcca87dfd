/* Test oracle of the local-alignment contract (include/ksw2_amd.h, ksw_ll_i16): a plain scalar int32 Smith-Waterman with Gotoh gaps
 * over the full matrix.  H(i,j) = max(0, H(i-1,j-1) + mat[t_i * m + q_j], E, F), a gap of length l costing gapo + l * gape; the best
 * cell is the largest H, then the smallest te, then the smallest qe; a best score of 0 gives (-1, -1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

int ll_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int *qe, int *te)
{
	const int64_t NEG = -((int64_t)1 << 40);
	int64_t *H, *E, best = 0;
	int i, j, bq = -1, bt = -1;
	*qe = *te = -1;
	if (qlen <= 0 || tlen <= 0) return 0;
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));      /* H(i-1, j) over j, then H(i, j) */
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));      /* E(i, j): gap along the target (vertical) */
	for (j = 0; j <= qlen; ++j) { H[j] = 0; E[j] = NEG; }
	for (i = 0; i < tlen; ++i) {                                      /* rows = target: row order is te order */
		int64_t diag = 0, F = NEG, hleft = 0;
		for (j = 0; j < qlen; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e, f;
			e = E[j + 1] - gape; if (up - gapo - gape > e) e = up - gapo - gape;
			f = F - gape; if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			h = diag + mat[target[i] * m + query[j]];
			if (e > h) h = e;
			if (f > h) h = f;
			if (h < 0) h = 0;
			E[j + 1] = e; F = f;
			diag = up; H[j + 1] = h; hleft = h;
			if (h > best) { best = h; bt = i; bq = j; }     /* strict: first in (te, qe) order among equals */
		}
	}
	free(H); free(E);
	*qe = bq; *te = bt;
	return (int)best;
}

/* n pairs from one arena: out[3 i ..] = score, qe, te */
void ll_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                     int m, const int8_t *mat, int gapo, int gape, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) {
		int qe, te;
		out[3 * i] = ll_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, &qe, &te);
		out[3 * i + 1] = qe; out[3 * i + 2] = te;
	}
}
