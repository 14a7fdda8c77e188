/* slfout.c -- the pieces of WriteOneLattice (HNet.c:530) that both lattice writers share (host/lattice.c: the decoder's lattices;
 * host/latrescore.c: lattices read back from files), so that the SLF text has one statement of each:
 *   htkamd_slf_put_word    "W=%-19s " with ReWriteString(.., NULL, ESCAPE_CHAR): never quoted, escapes where needed;
 *   htkamd_slf_sort_arcs   QSCmpArcs (HNet.c:466): by end node's output rank, then start node's, then arc number.
 */
#include <stdlib.h>
#include "../csrc/internal.h"
#include "htktext.h"

void htkamd_slf_put_word(FILE *f, const char *s)
{
   fputs("W=", f);
   htx_write_string(f, s, HTX_ESCAPE, -19);
   fputc(' ', f);
}

static const int *g_start, *g_end, *g_rank;        /* qsort context (the reference's `slat`) */

static int cmp_arcs(const void *v1, const void *v2)
{
   const int s1 = *(const int *)v1, s2 = *(const int *)v2;
   const int j = g_rank[g_end[s1]] - g_rank[g_end[s2]], k = g_rank[g_start[s1]] - g_rank[g_start[s2]];
   if (k == 0 && j == 0) return s1 - s2;
   return j == 0 ? k : j;
}

void htkamd_slf_sort_arcs(int *order, int nArcs, const int *arcStart, const int *arcEnd, const int *nodeRank)
{
   for (int i = 0; i < nArcs; i++) order[i] = i;
   g_start = arcStart; g_end = arcEnd; g_rank = nodeRank;
   qsort(order, (size_t)nArcs, sizeof(int), cmp_arcs);
   g_start = g_end = g_rank = NULL;
}
