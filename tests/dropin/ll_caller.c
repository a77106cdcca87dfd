/* Drop-in caller of the local-alignment pair (ksw2.h:92-93): compiled against a ksw2.h -- the reference's own, or include/ksw2_amd.h
 * with -DUSE_KSW2_AMD -- and linked against libksw2_amd.  Reads "m gapo gape", the m*m matrix, n, then per pair "qlen codes... tlen
 * codes..." from argv[1]; prints "score qe te" per pair.  The profile is released with free(), as a km == NULL caller does. */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#ifdef USE_KSW2_AMD
#include "ksw2_amd.h"
#else
#include "ksw2.h"
#endif

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
	if (!f || fscanf(f, "%d %d %d", &m, &gapo, &gape) != 3) return 2;
	mat = (int8_t*)malloc((size_t)m * m);
	for (i = 0; i < m * m; ++i) { if (fscanf(f, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
	if (fscanf(f, "%d", &n) != 1) return 2;
	for (i = 0; i < n; ++i) {
		int qlen, tlen, qe = -2, te = -2, score;
		uint8_t *q = read_seq(f, &qlen), *t = read_seq(f, &tlen);
		void *prof = ksw_ll_qinit(0, 2, qlen, q, m, mat);
		if (!prof) return 3;
		free(q);                               /* the profile holds its own copy */
		score = ksw_ll_i16(prof, tlen, t, gapo, gape, &qe, &te);
		free(prof);
		free(t);
		printf("%d %d %d\n", score, qe, te);
	}
	free(mat);
	fclose(f);
	return 0;
}
