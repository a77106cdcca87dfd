/* Test oracle of the two-piece suboptimal-score contract (include/ksw2_amd.h, ksw2amd_lld_sub_batch): the scalar Smith-Waterman of
 * tests/lls_oracle.c, rows = target, with the second pair of Gotoh gap states of tests/lld_oracle.c -- H(i,j) = max(0, H(i-1,j-1) +
 * mat[t_i * m + q_j], E, F, E2, F2), E / F under (gapo, gape), E2 / F2 under (gapo2, gape2), int64 and NOT clamped -- which also keeps
 * every row's maximum R(t) and the first column that reached it.  With (score, qe, te) the best cell (largest H, smallest te, smallest
 * qe) and d = excl >= 0 ? excl : ceil(score / smax): score2 = the largest R(t) over the rows with |t - te| > d, te2 the smallest such
 * row, qe2 the smallest column of that row with H == score2; (0, -1, -1) when no positive cell lies outside the window.  Compiled by
 * the tests. */
#include <stdint.h>
#include <stdlib.h>

void llds_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2,
                 int excl, int32_t *out)
{
	const int64_t NEG = -((int64_t)1 << 40);
	int64_t *H, *E, *E2, *R, best = 0, d, s2 = 0;
	int32_t *RC;
	int i, j, bq = -1, bt = -1, smax = -128, t2 = -1;
	out[0] = 0; out[1] = out[2] = -1; out[3] = 0; out[4] = out[5] = -1;
	if (qlen <= 0 || tlen <= 0) return;
	for (i = 0; i < m * m; ++i) if (mat[i] > smax) smax = mat[i];
	if (smax <= 0) return;
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	E2 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	R = (int64_t*)malloc(sizeof(int64_t) * (size_t)tlen);
	RC = (int32_t*)malloc(sizeof(int32_t) * (size_t)tlen);
	for (j = 0; j <= qlen; ++j) { H[j] = 0; E[j] = E2[j] = NEG; }
	for (i = 0; i < tlen; ++i) {
		int64_t diag = 0, F = NEG, F2 = NEG, hleft = 0;
		R[i] = 0; RC[i] = -1;
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
			if (h > R[i]) { R[i] = h; RC[i] = j; }
			if (h > best) { best = h; bt = i; bq = j; }
		}
	}
	out[0] = (int32_t)best; out[1] = bq; out[2] = bt;
	d = excl >= 0 ? excl : (best + smax - 1) / smax;
	for (i = 0; i < tlen; ++i) {
		const int64_t dt = (int64_t)i - bt;
		if (dt <= d && dt >= -d) continue;
		if (R[i] > s2) { s2 = R[i]; t2 = i; }
	}
	if (s2 > 0) { out[3] = (int32_t)s2; out[4] = RC[t2]; out[5] = t2; }
	free(H); free(E); free(E2); free(R); free(RC);
}

/* n pairs from one arena: out[6 i ..] = score, qe, te, score2, qe2, te2 */
void llds_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                       int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int excl, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) llds_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, gapo2, gape2, excl, out + 6 * i);
}
