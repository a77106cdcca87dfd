/* Test oracle of the overlap contract (include/ksw2_amd.h, ksw2amd_ov_batch / ksw2amd_ovd_batch): the formula restated in plain scalar
 * int64 with -infinity boundaries.  cost(l) = min(gapo + l * gape, gapo2 + l * gape2) (single piece: the caller passes the piece twice).
 * H(t, -1) = 0 for every t >= -1; H(-1, j) = 0 if ends & 1, else -cost(j + 1); H(t, j) = max(H(t-1, j-1) + mat[t_t * m + q_j], E, F, E2, F2)
 * with the four Gotoh states, no clamp at 0.  Candidates: (t, qlen - 1) for every t, and with ends & 2 (tlen - 1, j) for every j; the result
 * is the largest H, then the smallest te, then the smallest qe.  qlen <= 0: (0, -1, -1); tlen <= 0: ((ends & 1) ? 0 : -cost(qlen), qlen - 1,
 * -1).  Compiled by the tests. */
#include <stdint.h>
#include <stdlib.h>

static int64_t ov_cost(int64_t l, int gapo, int gape, int gapo2, int gape2)
{
	const int64_t a = gapo + l * gape, b = gapo2 + l * gape2;
	return a < b ? a : b;
}

int64_t ov_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2,
                  int ends, int *qe, int *te)
{
	const int64_t NEG = -((int64_t)1 << 50);
	int64_t *H, *E, *E2, best = NEG;
	int i, j, bt = -1, bq = -1;
	*qe = *te = -1;
	if (qlen <= 0) return 0;
	*qe = qlen - 1;
	if (tlen <= 0) return (ends & 1) ? 0 : -ov_cost(qlen, gapo, gape, gapo2, gape2);
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));      /* H(i-1, j-1) at [j], then H(i, j-1) */
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	E2 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(qlen + 1));
	H[0] = 0;
	for (j = 1; j <= qlen; ++j) { H[j] = (ends & 1) ? 0 : -ov_cost(j, gapo, gape, gapo2, gape2); E[j] = E2[j] = NEG; }
	for (i = 0; i < tlen; ++i) {
		int64_t diag = 0, F = NEG, F2 = NEG, hleft = 0;                /* column -1: H = 0, F = F2 = -infinity */
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
			E[j + 1] = e; F = f; E2[j + 1] = e2; F2 = f2;
			diag = up; H[j + 1] = h; hleft = h;
		}
		if (H[qlen] > best) { best = H[qlen]; bt = i; bq = qlen - 1; }      /* strict: the smallest te among equals */
	}
	if (ends & 2)                                                     /* row tlen - 1: te is the largest, so a larger H wins, or an equal one against the corner */
		for (j = 0; j < qlen; ++j)
			if (H[j + 1] > best || (H[j + 1] == best && bt == tlen - 1 && j < bq)) { best = H[j + 1]; bt = tlen - 1; bq = j; }
	free(H); free(E); free(E2);
	*te = bt; *qe = bq;
	return best;
}

/* n pairs from one arena: out[3 i ..] = score, qe, te */
void ov_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                     int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) {
		int qe, te;
		out[3 * i] = (int32_t)ov_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, gapo2, gape2, ends, &qe, &te);
		out[3 * i + 1] = qe; out[3 * i + 2] = te;
	}
}
