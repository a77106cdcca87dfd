/* Caller of the two-piece semi-global entries, compiled against include/ksw2_amd.h and linked against libksw2_amd.  Reads
 * "m gapo gape gapo2 gape2 flag", the m*m matrix, n, then per pair "qlen codes... tlen codes..." from argv[1]; prints per pair
 * "score qb qe tb te n_cigar cigar-words...", first from one ksw2amd_sgd_align_batch call, then -- after a line "single" -- from one
 * ksw2amd_sgd_align call per pair that reuses ONE result record (and its CIGAR buffer).  ksw2amd_sgd_batch and ksw2amd_sgd must return the
 * same score, qe and te (exit codes 6 and 7 otherwise). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

static void print_aln(const ksw2amd_laln_t *a)
{
	int k;
	printf("%d %d %d %d %d %d", a->score, a->qb, a->qe, a->tb, a->te, a->n_cigar);
	for (k = 0; k < a->n_cigar; ++k) printf(" %u", a->cigar[k]);
	printf("\n");
}

int main(int argc, char **argv)
{
	FILE *f = argc > 1 ? fopen(argv[1], "r") : 0;
	int m, gapo, gape, gapo2, gape2, flag, n, i, v, rc;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_lres_t *res;
	ksw2amd_laln_t *aln, one;
	if (!f || fscanf(f, "%d %d %d %d %d %d", &m, &gapo, &gape, &gapo2, &gape2, &flag) != 6) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)n + 1, sizeof(*pairs));
	res = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*res));
	aln = (ksw2amd_laln_t*)calloc((size_t)n + 1, sizeof(*aln));
	for (i = 0; i < n; ++i) {
		int ql, tl;
		pairs[i].query = read_seq(f, &ql); pairs[i].qlen = ql;
		pairs[i].target = read_seq(f, &tl); pairs[i].tlen = tl;
	}
	fclose(f);
	rc = ksw2amd_sgd_align_batch(0, m, mat, gapo, gape, gapo2, gape2, flag, n, pairs, aln);
	if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_sgd_align_batch: %d: %s\n", rc, ksw2amd_last_error()); return 3; }
	rc = ksw2amd_sgd_batch(m, mat, gapo, gape, gapo2, gape2, n, pairs, res);
	if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_sgd_batch: %d: %s\n", rc, ksw2amd_last_error()); return 3; }
	for (i = 0; i < n; ++i) {
		if (res[i].score != aln[i].score || res[i].qe != aln[i].qe || res[i].te != aln[i].te) return 6;
		print_aln(&aln[i]);
	}
	printf("single\n");
	memset(&one, 0, sizeof(one));
	for (i = 0; i < n; ++i) {
		void *prof = ksw_ll_qinit(0, 2, pairs[i].qlen, pairs[i].query, m, mat);
		int score, qe = -2, te = -2;
		if (!prof) return 4;
		score = ksw2amd_sgd_align(0, prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, flag, &one);
		if (score != one.score) return 5;
		if (ksw2amd_sgd(prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, &qe, &te) != one.score || qe != one.qe || te != one.te) return 7;
		print_aln(&one);
		free(prof);
	}
	for (i = 0; i < n; ++i) { free(aln[i].cigar); free((void*)pairs[i].query); free((void*)pairs[i].target); }
	free(one.cigar);
	free(pairs); free(res); free(aln); free(mat);
	return 0;
}
