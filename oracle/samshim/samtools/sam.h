/* oracle/samshim/samtools/sam.h -- TEST INFRASTRUCTURE ONLY: the four sam* calls of the reference's dwgsim_eval.c (see bam.h, samshim.c). */
#ifndef SAMSHIM_SAM_H
#define SAMSHIM_SAM_H
#include "bam.h"

typedef struct {
  bam_header_t *header;
  int mode;            /* 'r' text, 'b' BAM, 'w' writer */
  int own_header;
  FILE *fp;
  void *gz;
} samfile_t;

samfile_t *samopen(const char *fn, const char *mode, const void *aux);
int samread(samfile_t *fp, bam1_t *b);
int samwrite(samfile_t *fp, const bam1_t *b);
void samclose(samfile_t *fp);

#endif
