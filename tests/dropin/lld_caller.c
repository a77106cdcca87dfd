/* Caller of the two-piece local-alignment entries, compiled against include/ksw2_amd.h and linked against libksw2_amd.  Reads
 * "m gapo gape gapo2 gape2 flag", the m*m matrix, n, then per pair "qlen codes... tlen codes..." from argv[1]; prints per pair
 * "score qb qe tb te n_cigar cigar-words...", first from ksw2amd_lld_align_batch, then -- after a line "flat" -- from
 * ksw2amd_lld_align_batch_flat on a host arena built here, called TWICE into the same records (CIGAR buffers reused).  The two score
 * entries (ksw2amd_lld_batch, ksw2amd_lld_batch_flat) must agree with them (exit code 5 otherwise).  argv[2] = "pool": km is this
 * program's own pool; it exports krealloc / kfree (link with -rdynamic) and the last line is "pool <reallocs>". */
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
	void *km = argc > 2 && strcmp(argv[2], "pool") == 0 ? &pool : 0;
	int m, gapo, gape, gapo2, gape2, flag, n, i, v, rc;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_laln_t *aln, *faln;
	ksw2amd_lres_t *res, *fres;
	ksw2amd_lflat_t flat;
	uint64_t *qoff, *toff;
	int32_t *qlen, *tlen;
	uint8_t *base;
	size_t total = 3, pos = 3;
	if (!f || fscanf(f, "%d %d %d %d %d %d", &m, &gapo, &gape, &gapo2, &gape2, &flag) != 6) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)n + 1, sizeof(*pairs));
	aln = (ksw2amd_laln_t*)calloc((size_t)n + 1, sizeof(*aln));
	faln = (ksw2amd_laln_t*)calloc((size_t)n + 1, sizeof(*faln));
	res = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*res));
	fres = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*fres));
	qoff = (uint64_t*)calloc((size_t)n + 1, sizeof(*qoff)); toff = (uint64_t*)calloc((size_t)n + 1, sizeof(*toff));
	qlen = (int32_t*)calloc((size_t)n + 1, sizeof(*qlen)); tlen = (int32_t*)calloc((size_t)n + 1, sizeof(*tlen));
	for (i = 0; i < n; ++i) {
		int ql, tl;
		pairs[i].query = read_seq(f, &ql); pairs[i].qlen = ql;
		pairs[i].target = read_seq(f, &tl); pairs[i].tlen = tl;
		total += (size_t)ql + (size_t)tl + 2;
	}
	fclose(f);
	base = (uint8_t*)malloc(total);
	memset(base, 255, total);
	for (i = 0; i < n; ++i) {
		qoff[i] = pos; qlen[i] = pairs[i].qlen; memcpy(base + pos, pairs[i].query, (size_t)pairs[i].qlen); pos += (size_t)pairs[i].qlen + 1;
		toff[i] = pos; tlen[i] = pairs[i].tlen; memcpy(base + pos, pairs[i].target, (size_t)pairs[i].tlen); pos += (size_t)pairs[i].tlen + 1;
	}
	flat.base = base; flat.qoff = qoff; flat.toff = toff; flat.qlen = qlen; flat.tlen = tlen; flat.on_device = 0;
	rc = ksw2amd_lld_align_batch(km, m, mat, gapo, gape, gapo2, gape2, flag, n, pairs, aln);
	if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_lld_align_batch: %d: %s\n", rc, ksw2amd_last_error()); return 3; }
	for (i = 0; i < n; ++i) print_aln(&aln[i]);
	printf("flat\n");
	for (v = 0; v < 2; ++v) {
		rc = ksw2amd_lld_align_batch_flat(km, m, mat, gapo, gape, gapo2, gape2, flag, n, &flat, faln);
		if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_lld_align_batch_flat: %d: %s\n", rc, ksw2amd_last_error()); return 3; }
	}
	for (i = 0; i < n; ++i) print_aln(&faln[i]);
	if (ksw2amd_lld_batch(m, mat, gapo, gape, gapo2, gape2, n, pairs, res) != KSW2AMD_OK) return 4;
	if (ksw2amd_lld_batch_flat(m, mat, gapo, gape, gapo2, gape2, n, &flat, fres) != KSW2AMD_OK) return 4;
	for (i = 0; i < n; ++i)
		if (res[i].score != aln[i].score || res[i].qe != aln[i].qe || res[i].te != aln[i].te || memcmp(&res[i], &fres[i], sizeof(res[i])) != 0) return 5;
	for (i = 0; i < n; ++i) {
		if (km) { kfree(km, aln[i].cigar); kfree(km, faln[i].cigar); } else { free(aln[i].cigar); free(faln[i].cigar); }
		free((void*)pairs[i].query); free((void*)pairs[i].target);
	}
	if (km) printf("pool %ld\n", pool.n_realloc);
	free(pairs); free(aln); free(faln); free(res); free(fres); free(qoff); free(toff); free(qlen); free(tlen); free(base); free(mat);
	return 0;
}
