/* Caller of ksw2amd_ov_align_batch / ksw2amd_ov_align and ksw2amd_ovd_align_batch / ksw2amd_ovd_align, compiled against include/ksw2_amd.h
 * and linked against libksw2_amd.  Reads "m gapo gape gapo2 gape2 ends flag", the m*m matrix, n, then per pair "qlen codes... tlen codes..."
 * from argv[1]; prints per pair "score qb qe tb te n_cigar cigar-words...", first from one batch call, then -- after a line "single" -- from
 * one single-pair call per pair that reuses ONE result record (and its CIGAR buffer).  A further argument "dual" takes the two-piece entries
 * (else gapo2 / gape2 are read and ignored); "pool": km is this program's own pool; it exports krealloc / kfree (link with -rdynamic), the
 * library finds them at run time, and the last line is "pool <reallocs>". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "ksw2_amd.h"

typedef struct { long n_realloc, n_free; } pool_t;
void *krealloc(void *km, void *ptr, size_t size) { if (km) ++((pool_t*)km)->n_realloc; return realloc(ptr, size); }
void kfree(void *km, void *ptr) { if (km) ++((pool_t*)km)->n_free; free(ptr); }

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
	pool_t pool = { 0, 0 };
	void *km = 0;
	int m, gapo, gape, gapo2, gape2, ends, flag, n, i, v, rc, dual = 0;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_laln_t *aln, one;
	for (i = 2; i < argc; ++i) {
		if (strcmp(argv[i], "pool") == 0) km = &pool;
		if (strcmp(argv[i], "dual") == 0) dual = 1;
	}
	if (!f || fscanf(f, "%d %d %d %d %d %d %d", &m, &gapo, &gape, &gapo2, &gape2, &ends, &flag) != 7) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)n + 1, sizeof(*pairs));
	aln = (ksw2amd_laln_t*)calloc((size_t)n + 1, sizeof(*aln));
	for (i = 0; i < n; ++i) {
		int ql, tl;
		pairs[i].query = read_seq(f, &ql); pairs[i].qlen = ql;
		pairs[i].target = read_seq(f, &tl); pairs[i].tlen = tl;
	}
	fclose(f);
	rc = dual ? ksw2amd_ovd_align_batch(km, m, mat, gapo, gape, gapo2, gape2, ends, flag, n, pairs, aln)
	          : ksw2amd_ov_align_batch(km, m, mat, gapo, gape, ends, flag, n, pairs, aln);
	if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_ov%s_align_batch: %d: %s\n", dual ? "d" : "", rc, ksw2amd_last_error()); return 3; }
	for (i = 0; i < n; ++i) print_aln(&aln[i]);
	printf("single\n");
	memset(&one, 0, sizeof(one));
	for (i = 0; i < n; ++i) {
		void *prof = ksw_ll_qinit(km, 2, pairs[i].qlen, pairs[i].query, m, mat);
		int score;
		if (!prof) return 4;
		score = dual ? ksw2amd_ovd_align(km, prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, ends, flag, &one)
		             : ksw2amd_ov_align(km, prof, pairs[i].tlen, pairs[i].target, gapo, gape, ends, flag, &one);
		if (score != one.score) return 5;
		print_aln(&one);
		if (km) kfree(km, prof); else free(prof);
	}
	for (i = 0; i < n; ++i) {
		if (km) kfree(km, aln[i].cigar); else free(aln[i].cigar);
		free((void*)pairs[i].query); free((void*)pairs[i].target);
	}
	if (km) kfree(km, one.cigar); else free(one.cigar);
	if (km) printf("pool %ld\n", pool.n_realloc);
	free(pairs); free(aln); free(mat);
	return 0;
}
