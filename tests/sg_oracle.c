/* Test oracle of the semi-global contract (include/ksw2_amd.h, ksw2amd_sg_batch): the formula restated in plain scalar int64 with
 * -infinity boundaries.  H(t, -1) = 0 for every t >= -1, H(-1, j) = -(gapo + (j + 1) * gape), H(t, j) = max(H(t-1, j-1) + mat[t_t * m +
 * q_j], E, F) with Gotoh E / F, no clamp at 0; the result is the largest H(t, qlen - 1), the smallest such t, and qe = qlen - 1.
 * qlen <= 0: (0, -1, -1); tlen <= 0: (-(gapo + qlen * gape), qlen - 1, -1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

int64_t sg_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int *qe, int *te)
{
	const int64_t NEG = -((int64_t)1 << 50);
	int64_t *H, *E, best = NEG;
	int i, j, bt = -1;
	*qe = *te = -1;
	if (qlen <= 0) return 0;
	*qe = qlen - 1;
	if (tlen <= 0) return -((int64_t)gapo + (int64_t)qlen * gape);
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));      /* H(i-1, j-1) at [j], then H(i, j-1) */
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));      /* E(i, j-1) at [j]: gap along the target (vertical) */
	H[0] = 0;
	for (j = 1; j <= qlen; ++j) { H[j] = -((int64_t)gapo + (int64_t)j * gape); E[j] = NEG; }
	for (i = 0; i < tlen; ++i) {
		int64_t diag = 0, F = NEG, hleft = 0;                          /* column -1: H = 0, F = -infinity */
		for (j = 0; j < qlen; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e, f;
			e = E[j + 1] - gape; if (up - gapo - gape > e) e = up - gapo - gape;
			f = F - gape; if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			h = diag + mat[target[i] * m + query[j]];
			if (e > h) h = e;
			if (f > h) h = f;
			E[j + 1] = e; F = f;
			diag = up; H[j + 1] = h; hleft = h;
		}
		if (H[qlen] > best) { best = H[qlen]; bt = i; }                /* strict: the smallest te among equals */
	}
	free(H); free(E);
	*te = bt;
	return best;
}

/* n pairs from one arena: out[3 i ..] = score, qe, te */
void sg_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                     int m, const int8_t *mat, int gapo, int gape, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) {
		int qe, te;
		out[3 * i] = (int32_t)sg_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, &qe, &te);
		out[3 * i + 1] = qe; out[3 * i + 2] = te;
	}
}
