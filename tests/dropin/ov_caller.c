/* Caller of the overlap entries, compiled against include/ksw2_amd.h and linked against libksw2_amd.  Reads "m gapo gape gapo2 gape2", the
 * m*m matrix, n, then per pair "qlen codes... tlen codes..." from argv[1].  For ends = 0, 1, 2, 3 it prints a line "ends <e>" and per pair
 * "score qe te" from one ksw2amd_ov_batch call, then after a line "two-piece" the same from ksw2amd_ovd_batch.  The single-pair entries
 * ksw2amd_ov / ksw2amd_ovd, on a ksw_ll_qinit profile, must return the same (exit code 5 otherwise), and so must the flat entries on an arena
 * this program lays out (exit code 6).  argv[2] = "pool": the profiles are allocated in this program's own pool; it exports krealloc / kfree
 * (link with -rdynamic), the library finds them at run time, and the last line is "pool <reallocs>". */
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

int main(int argc, char **argv)
{
	FILE *f = argc > 1 ? fopen(argv[1], "r") : 0;
	pool_t pool = { 0, 0 };
	void *km = argc > 2 && strcmp(argv[2], "pool") == 0 ? &pool : 0;
	int m, gapo, gape, gapo2, gape2, n, i, v, rc, ends, dual;
	int8_t *mat;
	ksw2amd_lpair_t *pairs;
	ksw2amd_lres_t *res, *fres;
	ksw2amd_lflat_t flat;
	uint64_t *qoff, *toff, total = 0;
	int32_t *qlen, *tlen;
	uint8_t *arena;
	if (!f || fscanf(f, "%d %d %d %d %d", &m, &gapo, &gape, &gapo2, &gape2) != 5) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	pairs = (ksw2amd_lpair_t*)calloc((size_t)n + 1, sizeof(*pairs));
	res = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*res));
	fres = (ksw2amd_lres_t*)calloc((size_t)n + 1, sizeof(*fres));
	qoff = (uint64_t*)calloc((size_t)n + 1, sizeof(*qoff)); toff = (uint64_t*)calloc((size_t)n + 1, sizeof(*toff));
	qlen = (int32_t*)calloc((size_t)n + 1, sizeof(*qlen)); tlen = (int32_t*)calloc((size_t)n + 1, sizeof(*tlen));
	for (i = 0; i < n; ++i) {
		int ql, tl;
		pairs[i].query = read_seq(f, &ql); pairs[i].qlen = ql;
		pairs[i].target = read_seq(f, &tl); pairs[i].tlen = tl;
		qlen[i] = ql; tlen[i] = tl;
		qoff[i] = total; total += (uint64_t)(ql > 0 ? ql : 0);
		toff[i] = total; total += (uint64_t)(tl > 0 ? tl : 0);
	}
	fclose(f);
	arena = (uint8_t*)malloc((size_t)total + 1);
	for (i = 0; i < n; ++i) {
		if (qlen[i] > 0) memcpy(arena + qoff[i], pairs[i].query, (size_t)qlen[i]);
		if (tlen[i] > 0) memcpy(arena + toff[i], pairs[i].target, (size_t)tlen[i]);
	}
	memset(&flat, 0, sizeof(flat));
	flat.base = arena; flat.qoff = qoff; flat.toff = toff; flat.qlen = qlen; flat.tlen = tlen;
	for (dual = 0; dual < 2; ++dual) {
		if (dual) printf("two-piece\n");
		for (ends = 0; ends <= (KSW2AMD_OV_QBEG | KSW2AMD_OV_QEND); ++ends) {
			rc = dual ? ksw2amd_ovd_batch(m, mat, gapo, gape, gapo2, gape2, ends, n, pairs, res) : ksw2amd_ov_batch(m, mat, gapo, gape, ends, n, pairs, res);
			if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_ov%s_batch: %d: %s\n", dual ? "d" : "", rc, ksw2amd_last_error()); return 3; }
			rc = dual ? ksw2amd_ovd_batch_flat(m, mat, gapo, gape, gapo2, gape2, ends, n, &flat, fres) : ksw2amd_ov_batch_flat(m, mat, gapo, gape, ends, n, &flat, fres);
			if (rc != KSW2AMD_OK) { fprintf(stderr, "ksw2amd_ov%s_batch_flat: %d: %s\n", dual ? "d" : "", rc, ksw2amd_last_error()); return 3; }
			printf("ends %d\n", ends);
			for (i = 0; i < n; ++i) {
				void *prof = ksw_ll_qinit(km, 2, pairs[i].qlen, pairs[i].query, m, mat);
				int score, qe = -2, te = -2;
				if (!prof) return 4;
				score = dual ? ksw2amd_ovd(prof, pairs[i].tlen, pairs[i].target, gapo, gape, gapo2, gape2, ends, &qe, &te)
				             : ksw2amd_ov(prof, pairs[i].tlen, pairs[i].target, gapo, gape, ends, &qe, &te);
				if (score != res[i].score || qe != res[i].qe || te != res[i].te) return 5;
				if (fres[i].score != res[i].score || fres[i].qe != res[i].qe || fres[i].te != res[i].te) return 6;
				printf("%d %d %d\n", res[i].score, res[i].qe, res[i].te);
				kfree(km, prof);
			}
		}
	}
	if (km) printf("pool %ld\n", pool.n_realloc);
	for (i = 0; i < n; ++i) { free((void*)pairs[i].query); free((void*)pairs[i].target); }
	free(pairs); free(res); free(fres); free(qoff); free(toff); free(qlen); free(tlen); free(arena); free(mat);
	return 0;
}
