/* oracle/samshim/samtools/bam.h -- TEST INFRASTRUCTURE ONLY: what the reference's dwgsim_eval.c uses of samtools' bam.h, written here
 * from the SAM/BAM specification so that the UNMODIFIED dwgsim_eval.c compiles without the samtools sources (oracle/Makefile, target ref).
 * samshim.c has the functions and says what is not restated. */
#ifndef SAMSHIM_BAM_H
#define SAMSHIM_BAM_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* FLAG bits and CIGAR packing of the specification */
#define BAM_FPAIRED 1
#define BAM_FUNMAP 4
#define BAM_FREVERSE 16
#define BAM_FREAD1 64
#define BAM_CIGAR_SHIFT 4
#define BAM_CIGAR_MASK 0xf
#define BAM_CSOFT_CLIP 4
#define BAM_CHARD_CLIP 5

typedef struct {
  int32_t n_targets;
  char **target_name;
  size_t l_text;
  char *text;
} bam_header_t;

/* the 32 fixed bytes of a BAM record, unpacked */
typedef struct {
  int32_t tid, pos;
  uint32_t bin:16, qual:8, l_qname:8;
  uint32_t flag:16, n_cigar:16;
  int32_t l_qseq, mtid, mpos, isize;
} bam1_core_t;

/* data: QNAME with its NUL, the packed CIGAR, sequence, qualities, then the aux fields up to data_len, as in a BAM record.
 * line: text mode only, the record's line as it was read (samwrite prints it). */
typedef struct {
  bam1_core_t core;
  int data_len;
  uint8_t *data;
  char *line;
} bam1_t;

#define bam1_qname(b) ((char*)(b)->data)
#define bam1_cigar(b) ((uint32_t*)((b)->data + (b)->core.l_qname))
#define bam1_strand(b) (((b)->core.flag & BAM_FREVERSE) != 0)
#define bam1_aux(b) ((b)->data + (b)->core.l_qname + 4 * (b)->core.n_cigar + ((b)->core.l_qseq + 1) / 2 + (b)->core.l_qseq)

bam1_t *bam_init1(void);
void bam_destroy1(bam1_t *b);
uint8_t *bam_aux_get(const bam1_t *b, const char tag[2]);
int32_t bam_aux2i(const uint8_t *s);

#endif
