/* Caller of the flat local-alignment batches, compiled against include/ksw2_amd.h and linked against libksw2_amd: what a program does
 * that reads its sequences into ONE buffer.  Reads "m gapo gape flag", the m*m matrix, n, then per pair "qlen codes... tlen codes..."
 * from argv[1] into one arena (a pad byte that no matrix admits between the sequences); argv[2] = "host", "pinned" or "device".
 * Prints "score qe te" per pair from ksw2amd_ll_batch_flat, the line "align", then "score qb qe tb te n_cigar cigar..." per pair from
 * ksw2amd_ll_align_batch_flat, called twice on the same aln[] (the second call must reuse the CIGAR buffers: "reused 1"). */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "ksw2_amd.h"

int main(int argc, char **argv)
{
	FILE *f = argc > 1 ? fopen(argv[1], "r") : 0;
	const char *kind = argc > 2 ? argv[2] : "host";
	int m, gapo, gape, flag, n, i, k, v, reused = 1, rc;
	size_t cap = 1 << 16, used = 3;
	uint8_t *arena = (uint8_t*)malloc(cap);
	void *dev = 0;
	int8_t *mat;
	uint64_t *off;
	int32_t *len;
	ksw2amd_lflat_t in;
	ksw2amd_lres_t *res;
	ksw2amd_laln_t *aln;
	uint32_t **first;
	if (!f || !arena || fscanf(f, "%d %d %d %d", &m, &gapo, &gape, &flag) != 4) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	off = (uint64_t*)malloc(sizeof(*off) * (size_t)(2 * n + 1));
	len = (int32_t*)malloc(sizeof(*len) * (size_t)(2 * n + 1));
	memset(arena, 0xff, 3);
	for (i = 0; i < 2 * n; ++i) {                  /* query 0, target 0, query 1, ... */
		if (fscanf(f, "%d", &len[i]) != 1) return 2;
		while (used + (size_t)len[i] + 1 > cap) { cap *= 2; if (!(arena = (uint8_t*)realloc(arena, cap))) return 2; }
		off[i] = used;
		for (k = 0; k < len[i]; ++k) { if (fscanf(f, "%d", &v) != 1) return 2; arena[used++] = (uint8_t)v; }
		arena[used++] = 0xff;
	}
	fclose(f);
	{	/* the library takes strided views of nothing: split the interleaved arrays */
		uint64_t *qo = (uint64_t*)malloc(sizeof(*qo) * (size_t)(2 * n + 2)), *to = qo + n;
		int32_t *ql = (int32_t*)malloc(sizeof(*ql) * (size_t)(2 * n + 2)), *tl = ql + n;
		for (i = 0; i < n; ++i) { qo[i] = off[2 * i]; to[i] = off[2 * i + 1]; ql[i] = len[2 * i]; tl[i] = len[2 * i + 1]; }
		in.qoff = qo; in.toff = to; in.qlen = ql; in.tlen = tl;
	}
	in.base = arena; in.on_device = 0;
	if (!strcmp(kind, "pinned")) { if (ksw2amd_host_register(arena, used) != KSW2AMD_OK) { fprintf(stderr, "%s\n", ksw2amd_last_error()); return 3; } }
	else if (!strcmp(kind, "device")) {
		if (!(dev = ksw2amd_device_alloc(used)) || ksw2amd_device_upload(dev, arena, used) != KSW2AMD_OK) { fprintf(stderr, "%s\n", ksw2amd_last_error()); return 3; }
		memset(arena, 0xff, used);             /* the host copy is not what is aligned */
		in.base = (const uint8_t*)dev; in.on_device = 1;
	}
	res = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*res));
	aln = (ksw2amd_laln_t*)calloc((size_t)n + 1, sizeof(*aln));
	first = (uint32_t**)calloc((size_t)n + 1, sizeof(*first));
	if ((rc = ksw2amd_ll_batch_flat(m, mat, gapo, gape, n, &in, res)) != KSW2AMD_OK) { fprintf(stderr, "%d %s\n", rc, ksw2amd_last_error()); return 4; }
	for (i = 0; i < n; ++i) printf("%d %d %d\n", res[i].score, res[i].qe, res[i].te);
	if ((rc = ksw2amd_ll_align_batch_flat(0, m, mat, gapo, gape, flag, n, &in, aln)) != KSW2AMD_OK) { fprintf(stderr, "%d %s\n", rc, ksw2amd_last_error()); return 4; }
	for (i = 0; i < n; ++i) first[i] = aln[i].cigar;
	if ((rc = ksw2amd_ll_align_batch_flat(0, m, mat, gapo, gape, flag, n, &in, aln)) != KSW2AMD_OK) { fprintf(stderr, "%d %s\n", rc, ksw2amd_last_error()); return 4; }
	printf("align\n");
	for (i = 0; i < n; ++i) {
		printf("%d %d %d %d %d %d", aln[i].score, aln[i].qb, aln[i].qe, aln[i].tb, aln[i].te, aln[i].n_cigar);
		for (k = 0; k < aln[i].n_cigar; ++k) printf(" %u", aln[i].cigar[k]);
		printf("\n");
		if (aln[i].cigar != first[i]) reused = 0;
		free(aln[i].cigar);
	}
	printf("reused %d\n", reused);
	if (!strcmp(kind, "pinned")) ksw2amd_host_unregister(arena);
	if (dev) ksw2amd_device_free(dev);
	return 0;
}
