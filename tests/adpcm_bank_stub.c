/* A stand-in for the one-channel banks behind the IMA and OKI ADPCM objects (csrc/shim_adpcm.c), for the host-side
 * transcript test of tests/test_adpcm.py: the shim + this file + tests/c_callers/adpcm_objects.c under
 * -fsanitize=address,undefined; no GPU.  It keeps no signal state.  Every call prints itself with its scalar arguments,
 * touches exactly the memory the real bank touches (a whole row of the stride it is given), and answers with something
 * trivial and deterministic: it counts two codes a byte and fills its row from a sum of its input.  The driver sets
 * stub_fail_create to make the k-th create from now fail.  Test code only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spangpu.h"

int stub_fail_create = 0;
int stub_live = 0;              /* banks created and not yet destroyed */

typedef struct
{
    int id;
    int a;                      /* ima: variant; oki: bit rate */
    int b;                      /* ima: chunk size */
} bank_t;

struct spangpu_ima_adpcm_s { bank_t k; };
struct spangpu_oki_adpcm_s { bank_t k; };

static int next_id = 0;

static void *make(const char *what)
{
    bank_t *k;

    if (stub_fail_create > 0  &&  --stub_fail_create == 0)
    {
        printf("  bank: %s fails\n", what);
        return NULL;
    }
    if ((k = (bank_t *) calloc(1, sizeof(*k))) == NULL)
        abort();
    k->id = ++next_id;
    stub_live++;
    printf("  bank: %s -> #%d\n", what, k->id);
    return k;
}

static void unmake(const char *what, void *bank)
{
    printf("  bank: %s(#%d)\n", what, ((bank_t *) bank)->id);
    stub_live--;
    free(bank);
}

static unsigned sum_of(const void *p, long long bytes)
{
    const uint8_t *b = (const uint8_t *) p;
    unsigned s = 0;
    long long i;

    for (i = 0;  i < bytes;  i++)
        s = s*31 + b[i];
    return s;
}

/* a codec's row: the whole stride, from a sum of the whole input row */
static void code_row(void *out, long long out_bytes, const void *in, long long in_bytes)
{
    const unsigned s = sum_of(in, in_bytes);
    long long i;

    for (i = 0;  i < out_bytes;  i++)
        ((uint8_t *) out)[i] = (uint8_t) (s + 7*i + 1);
}

const char *spangpu_last_error(void) { return "stub bank"; }

#define FAMILY(fam, CREATE_ARGS, CREATE_FMT, CREATE_VALUES, SET)                                                        \
int spangpu_##fam##_create CREATE_ARGS                                                                                  \
{                                                                                                                       \
    char what[96];                                                                                                      \
                                                                                                                        \
    sprintf(what, #fam "_create(dev %d, ch %d, " CREATE_FMT ", n %d)", device, n_channels, CREATE_VALUES, n);           \
    if ((*bank = (spangpu_##fam##_t *) make(what)) == NULL)                                                             \
        return SPANGPU_ERR_NO_DEVICE;                                                                                   \
    SET;                                                                                                                \
    return SPANGPU_OK;                                                                                                  \
}                                                                                                                       \
                                                                                                                        \
void spangpu_##fam##_destroy(spangpu_##fam##_t *bank) { unmake(#fam "_destroy", bank); }                                \
                                                                                                                        \
long long spangpu_##fam##_encode_capacity(const spangpu_##fam##_t *bank, int samples)                                   \
{                                                                                                                       \
    printf("  bank: " #fam "_encode_capacity(#%d, %d)\n", bank->k.id, samples);                                         \
    return samples/2 + 5;                                                                                               \
}                                                                                                                       \
                                                                                                                        \
long long spangpu_##fam##_decode_capacity(const spangpu_##fam##_t *bank, int bytes)                                     \
{                                                                                                                       \
    printf("  bank: " #fam "_decode_capacity(#%d, %d)\n", bank->k.id, bytes);                                           \
    return 2*(long long) bytes + 1;                                                                                     \
}                                                                                                                       \
                                                                                                                        \
int spangpu_##fam##_encode(spangpu_##fam##_t *bank, const void *amp,   int amp_mem_kind, long long amp_stride_bytes,   \
                           const int32_t *lens, int max_samples, uint8_t *codes, int codes_mem_kind,                   \
                           long long codes_stride_bytes, int32_t *bytes_out)                                            \
{                                                                                                                       \
    code_row(codes, codes_stride_bytes, amp, amp_stride_bytes);                                                         \
    bytes_out[0] = (max_samples + 1)/2;                                                                                 \
    printf("  bank: " #fam "_encode(#%d, mem %d, in stride %lld, lens %s, samples %d, mem %d, out stride %lld) -> %d\n", bank->k.id,     \
           amp_mem_kind, amp_stride_bytes, lens  ?  "given"  :  "NULL", max_samples, codes_mem_kind, codes_stride_bytes, (int) bytes_out[0]);   \
    return SPANGPU_OK;                                                                                                  \
}                                                                                                                       \
                                                                                                                        \
int spangpu_##fam##_decode(spangpu_##fam##_t *bank, const uint8_t *codes, int codes_mem_kind, long long codes_stride_bytes,      \
                           const int32_t *lens, int max_bytes, void *amp, int amp_mem_kind, long long amp_stride_bytes,         \
                           int32_t *samples_out)                                                                        \
{                                                                                                                       \
    code_row(amp, amp_stride_bytes, codes, codes_stride_bytes);                                                         \
    samples_out[0] = 2*max_bytes;                                                                                       \
    printf("  bank: " #fam "_decode(#%d, mem %d, in stride %lld, lens %s, bytes %d, mem %d, out stride %lld) -> %d\n", bank->k.id,       \
           codes_mem_kind, codes_stride_bytes, lens  ?  "given"  :  "NULL", max_bytes, amp_mem_kind, amp_stride_bytes, (int) samples_out[0]);   \
    return SPANGPU_OK;                                                                                                  \
}

#define IMA_CREATE_ARGS (spangpu_ima_adpcm_t **bank, int device, int n_channels, const int32_t *variants, const int32_t *chunk_sizes, int n)
#define IMA_VALUES      (int) variants[0], (int) chunk_sizes[0]
#define OKI_CREATE_ARGS (spangpu_oki_adpcm_t **bank, int device, int n_channels, const int32_t *bit_rates, int n)

FAMILY(ima_adpcm, IMA_CREATE_ARGS, "variant %d, chunk %d", IMA_VALUES, ((*bank)->k.a = variants[0], (*bank)->k.b = chunk_sizes[0]))
FAMILY(oki_adpcm, OKI_CREATE_ARGS, "rate %d", (int) bit_rates[0], (*bank)->k.a = bit_rates[0])
