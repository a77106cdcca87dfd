/* Test oracle of the overlap contract with the start cell (include/ksw2_amd.h, ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch): plain scalar
 * int64 with -infinity boundaries, no bias, no clamp.  (score, qe, te) is tests/ov_oracle.c's.  The start: one global matrix of
 * reverse(query[0..qe]) against reverse(target[0..te]) under cost(l) = min(gapo + l * gape, gapo2 + l * gape2) -- cell (i, j) of it is
 * G(te - i, qe - j), the global score of query[qe-j..qe] against target[te-i..te] -- whose last column holds the candidates (tb, 0) and whose
 * last row holds the candidates (0, qb); the empty intervals are its boundary, G(te + 1, 0) = -cost(qe + 1) and G(0, qe + 1) = -cost(te + 1).
 * The candidates are walked in the contract's order -- the largest tb first, then the largest qb -- and the first one equal to the score is
 * the answer; `found` says whether any was.  Compiled by the tests together with tests/ov_oracle.c. */
#include <stdint.h>
#include <stdlib.h>

int64_t ov_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2,
                  int ends, int *qe, int *te);

static int64_t ova_cost(int64_t l, int gapo, int gape, int gapo2, int gape2)
{
	const int64_t a = gapo + l * gape, b = gapo2 + l * gape2;
	return a < b ? a : b;
}

/* out: score, qb, qe, tb, te, found */
void ova_oracle(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2,
                int ends, int32_t *out)
{
	const int64_t NEG = -((int64_t)1 << 50);
	int qe, te, i, j, nr, nc;
	const int64_t sc = ov_oracle(qlen, query, tlen, target, m, mat, gapo, gape, gapo2, gape2, ends, &qe, &te);
	int64_t *H, *E, *E2, *last;
	out[0] = (int32_t)sc; out[1] = -1; out[2] = qe; out[3] = -1; out[4] = te; out[5] = 1;
	if (qlen <= 0) return;
	if (tlen <= 0) { out[1] = (ends & 1) ? qlen : 0; out[3] = 0; return; }
	nr = te + 1; nc = qe + 1;
	H = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nc + 1));
	E = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nc + 1));
	E2 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nc + 1));
	last = (int64_t*)malloc(sizeof(int64_t) * (size_t)nr);             /* the last column, row by row */
	H[0] = 0;
	for (j = 1; j <= nc; ++j) { H[j] = -ova_cost(j, gapo, gape, gapo2, gape2); E[j] = E2[j] = NEG; }
	for (i = 0; i < nr; ++i) {
		int64_t diag = H[0], F = NEG, F2 = NEG, hleft = -ova_cost(i + 1, gapo, gape, gapo2, gape2);
		H[0] = hleft;
		for (j = 0; j < nc; ++j) {
			const int64_t up = H[j + 1];
			int64_t h, e, f, e2, f2;
			e = E[j + 1] - gape; if (up - gapo - gape > e) e = up - gapo - gape;
			f = F - gape; if (hleft - gapo - gape > f) f = hleft - gapo - gape;
			e2 = E2[j + 1] - gape2; if (up - gapo2 - gape2 > e2) e2 = up - gapo2 - gape2;
			f2 = F2 - gape2; if (hleft - gapo2 - gape2 > f2) f2 = hleft - gapo2 - gape2;
			h = diag + mat[target[te - i] * m + query[qe - j]];
			if (e > h) h = e;
			if (f > h) h = f;
			if (e2 > h) h = e2;
			if (f2 > h) h = f2;
			E[j + 1] = e; F = f; E2[j + 1] = e2; F2 = f2;
			diag = up; H[j + 1] = h; hleft = h;
		}
		last[i] = H[nc];
	}
	/* H[] is now the last row: H[j + 1] = G(0, qe - j), H[0] = G(0, qe + 1) */
	out[5] = 0;
	if (-ova_cost(nc, gapo, gape, gapo2, gape2) == sc) { out[1] = 0; out[3] = te + 1; out[5] = 1; }
	for (i = 0; !out[5] && i < nr - 1; ++i)                             /* tb = te - i > 0 */
		if (last[i] == sc) { out[1] = 0; out[3] = te - i; out[5] = 1; }
	if (!out[5] && (ends & 1))                                         /* row 0: qb = qe + 1 down to 1 */
		for (j = -1; !out[5] && j < nc - 1; ++j)
			if (H[j + 1] == sc) { out[1] = qe - j; out[3] = 0; out[5] = 1; }
	if (!out[5] && H[nc] == sc) { out[1] = 0; out[3] = 0; out[5] = 1; }
	free(H); free(E); free(E2); free(last);
}

/* n pairs from one arena: out[6 i ..] = score, qb, qe, tb, te, found */
void ova_oracle_batch(int n, const uint8_t *base, const int64_t *qoff, const int32_t *qlen, const int64_t *toff, const int32_t *tlen,
                      int m, const int8_t *mat, int gapo, int gape, int gapo2, int gape2, int ends, int32_t *out)
{
	int i;
	for (i = 0; i < n; ++i) ova_oracle(qlen[i], base + qoff[i], tlen[i], base + toff[i], m, mat, gapo, gape, gapo2, gape2, ends, out + 6 * i);
}
