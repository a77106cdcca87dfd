/* C caller of the two-piece suboptimal-score entry and the two-piece single-pair entries, compiled against the public header
 * include/ksw2_amd.h and linked against libksw2_amd.  Reads "m gapo gape gapo2 gape2 excl", the m*m matrix, n, then per pair "qlen
 * codes... tlen codes..." from argv[1]; prints per pair "score qe te score2 qe2 te2" from ksw2amd_lld_sub_batch (all pairs in one
 * call), then the same from ksw2amd_lld_sub on a ksw_ll_qinit profile, then "score qe te" of ksw2amd_lld followed by "score qb tb" of
 * ksw2amd_lld_align on the same profile. */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
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
	int m, gapo, gape, gapo2, gape2, excl, n, i, v;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_lres_t *res;
	ksw2amd_lsub_t *sub;
	if (!f || fscanf(f, "%d %d %d %d %d %d", &m, &gapo, &gape, &gapo2, &gape2, &excl) != 6) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)n + 1, sizeof(*pairs));
	res = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*res));
	sub = (ksw2amd_lsub_t*)calloc((size_t)n + 1, sizeof(*sub));
	for (i = 0; i < n; ++i) { pairs[i].query = read_seq(f, &pairs[i].qlen); pairs[i].target = read_seq(f, &pairs[i].tlen); }
	if (ksw2amd_lld_sub_batch(m, mat, gapo, gape, gapo2, gape2, excl, n, pairs, res, sub) != KSW2AMD_OK) { fprintf(stderr, "%s\n", ksw2amd_last_error()); return 3; }
	for (i = 0; i < n; ++i) printf("%d %d %d %d %d %d\n", res[i].score, res[i].qe, res[i].te, sub[i].score2, sub[i].qe2, sub[i].te2);
	for (i = 0; i < n; ++i) {
		int qe = -2, te = -2, score;
		ksw2amd_lsub_t s;
		void *prof = ksw_ll_qinit(0, 2, pairs[i].qlen, pairs[i].query, m, mat);
		if (!prof) return 3;
		score = ksw2amd_lld_sub(prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, excl, &qe, &te, &s);
		free(prof);
		printf("%d %d %d %d %d %d\n", score, qe, te, s.score2, s.qe2, s.te2);
	}
	for (i = 0; i < n; ++i) {
		int qe = -2, te = -2, score, ascore;
		ksw2amd_laln_t a;
		void *prof = ksw_ll_qinit(0, 2, pairs[i].qlen, pairs[i].query, m, mat);
		if (!prof) return 3;
		memset(&a, 0, sizeof(a));
		score = ksw2amd_lld(prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, &qe, &te);
		ascore = ksw2amd_lld_align(0, prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, 0, &a);
		if (a.qe != qe || a.te != te || (ascore > 0) != (a.n_cigar > 0)) return 4;
		free(a.cigar);
		free(prof);
		printf("%d %d %d %d %d %d\n", score, qe, te, ascore, a.qb, a.tb);
	}
	fclose(f);
	return 0;
}
