/* ref_strings.c -- what the REFERENCE's text routines make of given bytes (TEST INFRASTRUCTURE).
 *
 * Compiled by oracle/Makefile against the reference's headers where they lie and linked with oracle/_ref/HTKLib.a; no reference source
 * text is copied into this file.  tests/golden/make_htktext_golden.py runs it and records the answers.
 *
 *   ref_strings read FILE     ReadString until the file ends: per call a line "T <hex of the string> <wasQuoted>" or "F"
 *   ref_strings write HEX     ReWriteString of the bytes HEX under q = 0, ', " and \: four lines of hex
 *   ref_strings labels FILE   LOpen (HTK format): per label of the first list "<hex of the name> <score %.9g> <start %.0f> <end %.0f>"
 *   ref_strings dict FILE     ReadDict: per pronunciation "<hex word> <pnum> <hex outsym or -> <log prob %.9g> <hex phone>..."
 * A refusal of the reference (HError) ends the process with its message on stderr and a non-zero status.
 */
#include "HShell.h"
#include "HMem.h"
#include "HMath.h"
#include "HWave.h"
#include "HLabel.h"
#include "HDict.h"

static void hex(const char *s)
{
   if (!*s) printf("''");
   for (; *s; s++) printf("%02x", (unsigned char)*s);
}

int main(int argc, char *argv[])
{
   static MemHeap heap;
   char buf[MAXSTRLEN * 4 + 8], in[MAXSTRLEN];
   const char *mode, *arg;
   static const char quotes[4] = {0, '\'', '"', '\\'};
   int i;

   if (argc != 3) { fprintf(stderr, "usage: ref_strings read|write|labels|dict ARG\n"); return 2; }
   mode = argv[1]; arg = argv[2];
   argc = 1;
   if (InitShell(argc, argv, "ref_strings", "") < SUCCESS) HError(9999, "InitShell");
   InitMem(); InitMath(); InitWave(); InitLabel(); InitDict();
   CreateHeap(&heap, "store", MSTAK, 1, 1.0, 50000, 500000);

   if (!strcmp(mode, "read")) {
      Source src;
      if (InitSource((char *)arg, &src, NoFilter) < SUCCESS) HError(9999, "cannot open %s", arg);
      for (;;) {
         int c;
         if (ReadString(&src, buf)) { printf("T "); hex(buf); printf(" %d\n", src.wasQuoted ? 1 : 0); continue; }
         printf("F\n");
         c = GetCh(&src);
         if (c == EOF) break;
         UnGetCh(c, &src);
      }
      CloseSource(&src);
   } else if (!strcmp(mode, "write")) {
      size_t n = strlen(arg) / 2;
      for (i = 0; i < (int)n && i < MAXSTRLEN - 1; i++) { unsigned v; sscanf(arg + 2 * i, "%2x", &v); in[i] = (char)v; }
      in[i] = 0;
      for (i = 0; i < 4; i++) { hex(ReWriteString(in, buf, quotes[i])); printf("\n"); }
   } else if (!strcmp(mode, "labels")) {
      Transcription *t = LOpen(&heap, (char *)arg, HTK);
      LabList *ll = GetLabelList(t, 1);
      const int n = CountLabs(ll);
      for (i = 1; i <= n; i++) {
         LLink l = GetLabN(ll, i);
         hex(l->labid->name); printf(" %.9g %.0f %.0f\n", l->score, l->start, l->end);
      }
   } else if (!strcmp(mode, "dict")) {
      Vocab voc;
      Word w; Pron p;
      InitVocab(&voc);
      if (ReadDict((char *)arg, &voc) < SUCCESS) HError(9999, "ReadDict failed");
      for (i = 0; i < VHASHSIZE; i++)
         for (w = voc.wtab[i]; w != NULL; w = w->next)
            for (p = w->pron; p != NULL; p = p->next) {
               int k;
               hex(w->wordName->name); printf(" %d ", p->pnum);
               if (p->outSym) hex(p->outSym->name); else printf("-");
               printf(" %.9g", p->prob);
               for (k = 0; k < p->nphones; k++) { printf(" "); hex(p->phones[k]->name); }
               printf("\n");
            }
   } else { fprintf(stderr, "ref_strings: unknown mode %s\n", mode); return 2; }
   return 0;
}
