/* Caller of the semi-global entries, compiled against include/ksw2_amd.h and linked against libksw2_amd.  Reads "m gapo gape", the m*m
 * matrix, n, then per pair "qlen codes... tlen codes..." from argv[1]; prints "score qe te" per pair twice: from ksw2amd_sg on a
 * ksw_ll_qinit profile (released with free(), as a km == NULL caller does), then from one ksw2amd_sg_batch call over all pairs. */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "ksw2_amd.h"

static uint8_t *read_seq(FILE *f, int *len)
{
	int i, v;
	uint8_t *s;
	if (fscanf(f, "%d", len) != 1) exit(2);
	s = (uint8_t*)malloc((size_t)(*len > 0 ? *len : 1));
	for (i = 0; i < *len; ++i) { if (fscanf(f, "%d", &v) != 1) exit(2); s[i] = (uint8_t)v; }
	return s;
}

int main(int argc, char **argv)
{
	FILE *f = argc > 1 ? fopen(argv[1], "r") : 0;
	int m, gapo, gape, n, i, v;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_lres_t *res;
	if (!f || fscanf(f, "%d %d %d", &m, &gapo, &gape) != 3) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)(n > 0 ? n : 1), sizeof(*pairs));
	res = (ksw2amd_lres_t*)calloc((size_t)(n > 0 ? n : 1), sizeof(*res));
	for (i = 0; i < n; ++i) {
		int qlen, tlen, qe = -2, te = -2, score;
		uint8_t *q = read_seq(f, &qlen), *t = read_seq(f, &tlen);
		void *prof = ksw_ll_qinit(0, 2, qlen, q, m, mat);
		if (!prof) return 3;
		score = ksw2amd_sg(prof, tlen, t, gapo, gape, &qe, &te);
		free(prof);
		printf("%d %d %d\n", score, qe, te);
		pairs[i].query = q; pairs[i].qlen = qlen; pairs[i].target = t; pairs[i].tlen = tlen;
	}
	if (ksw2amd_sg_batch(m, mat, gapo, gape, n, pairs, res) != KSW2AMD_OK) { fprintf(stderr, "%s\n", ksw2amd_last_error()); return 4; }
	for (i = 0; i < n; ++i) {
		printf("%d %d %d\n", res[i].score, res[i].qe, res[i].te);
		free((void*)pairs[i].query); free((void*)pairs[i].target);
	}
	free(pairs); free(res); free(mat);
	fclose(f);
	return 0;
}
