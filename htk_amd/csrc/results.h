/* results.h -- the scorer's handle as host/results.c (names, references, text) and csrc/results.hip (the device side) share it. */
#ifndef HTKAMD_RESULTS_H
#define HTKAMD_RESULTS_H
#include "internal.h"

#ifdef __cplusplus
extern "C" {
#endif

struct htkamd_results {
   char *nullName;
   int ignoreCase, strip, nist;
   int nEquiv; char **eqClass, **eqLabel;
   int nList;                              /* ids 1 .. nList: the label list */
   int nNames, capNames; char **name;      /* id -> name, [0] the null class */
   int *hash; int hashCap;                 /* open addressing over `name`: id or -1 */
   int nRefs, capRefs; char **refName; int *refOff;   /* refOff [nRefs + 1] into refIds */
   int *refIds; int capRefIds;
   int refsOnDevice;                       /* references the device copy holds */
   void *dev;                              /* csrc/results.hip's buffers, and how to free them (set where they are made: the host code links without the device side) */
   void (*devFree)(void *);
   double kernelMs;
};

#ifdef __cplusplus
}
#endif
#endif
