// tone_cadence.hip -- super-tone cadences matched on the device: the matcher's kernels over a launch's block records, its
// buffers and the spangpu_bank_cadence_* calls.  cadence_dev.hpp has the walk (the streaming kernel's epilogue runs it too).

#include <stdlib.h>
#include <string.h>
#include <vector>

#include "tone_cadence.hpp"

using namespace spg;

__global__ __launch_bounds__(256) void cadence_init_kernel(int32_t *st, int n_ch, int first, int n)
{
    const int i = (int) (blockIdx.x*256 + threadIdx.x);
    if (i >= n)
        return;
    const int ch = first + i;
    for (int w = 0;  w < kCadWords;  w++)
        st[(size_t) w*n_ch + ch] = (w == 3  ||  w >= 4 + kCadHistory)  ?  0  :  -1;
}

// A launch of its own over the records of the last detector launch (whatever kernel made them).
__global__ __launch_bounds__(256) void cadence_kernel(const uint32_t *__restrict__ rec, int n_ch, int maxb, const CadenceArgs A)
{
    __shared__ uint32_t wg_events;
    __shared__ uint32_t wg_at;
    if (threadIdx.x == 0)
        wg_events = 0;
    __syncthreads();
    // lanes past the end of the bank walk the last channel again and write nothing (they have barriers to keep)
    const bool active = ((int) (blockIdx.x*256 + threadIdx.x) < n_ch);
    const int ch = active  ?  (int) (blockIdx.x*256 + threadIdx.x)  :  n_ch - 1;
    // the records of a 160-sample frame (one or two blocks) are asked for along with the state: one trip to memory in all
    const uint32_t rec0 = (maxb > 0)  ?  rec[ch]  :  0;
    const uint32_t rec1 = (maxb > 1)  ?  rec[(size_t) n_ch + ch]  :  0;
    const int n_ev = cadence_walk(A, ch, n_ch, maxb, rec0, rec1, rec, active);
    // the compact list: the workgroup takes room for all its events with one atomic on the list's counter (thousands of lanes
    // adding to one address cost more than the rest of the kernel), each channel a piece of that
    const uint32_t mine = (n_ev > 0)  ?  atomicAdd(&wg_events, (uint32_t) n_ev)  :  0;
    __syncthreads();
    if (threadIdx.x == 0  &&  wg_events > 0)
        wg_at = atomicAdd(A.list + A.which, wg_events);
    if (blockIdx.x == 0  &&  threadIdx.x == 0)
        A.list[A.which ^ 1] = 0;                // the next launch's counter (it starts when this one is over)
    __syncthreads();
    if (n_ev > 0)
        cadence_list_copy(A, ch, n_ch, n_ev, wg_at + mine);
}

// The compact list from the slot arrays, for launches whose detector kernel matched the cadences itself.
__global__ __launch_bounds__(256) void cadence_list_kernel(int n_ch, const CadenceArgs A)
{
    __shared__ uint32_t wg_events;
    __shared__ uint32_t wg_at;
    if (threadIdx.x == 0)
        wg_events = 0;
    __syncthreads();
    const int ch = (int) (blockIdx.x*256 + threadIdx.x);
    const int n_ev = (ch < n_ch)  ?  A.count[ch]  :  0;
    const uint32_t mine = (n_ev > 0)  ?  atomicAdd(&wg_events, (uint32_t) n_ev)  :  0;
    __syncthreads();
    if (threadIdx.x == 0  &&  wg_events > 0)
        wg_at = atomicAdd(A.list + A.which, wg_events);
    if (blockIdx.x == 0  &&  threadIdx.x == 0)
        A.list[A.which ^ 1] = 0;
    __syncthreads();
    if (n_ev > 0)
        cadence_list_copy(A, ch, n_ch, n_ev, wg_at + mine);
}

void cadence_free(Cadence *c)
{
    if (c == nullptr)
        return;
    if (c->d_first) (void) hipFree(c->d_first);
    if (c->d_elem) (void) hipFree(c->d_elem);
    if (c->d_state) (void) hipFree(c->d_state);
    if (c->d_ev) (void) hipFree(c->d_ev);
    if (c->d_count) (void) hipFree(c->d_count);
    if (c->h_ev) (void) hipHostFree(c->h_ev);
    if (c->h_count) (void) hipHostFree(c->h_count);
    if (c->d_list) (void) hipFree(c->d_list);
    if (c->h_list) (void) hipHostFree(c->h_list);
    free(c);
}

// Event buffers for launches of up to `slots` slots per channel.
static int cadence_event_room(spangpu_bank_t *b, int slots)
{
    Cadence *c = b->cad;
    if (slots <= c->slots_cap)
        return SPANGPU_OK;
    SPG_TRY(hipStreamSynchronize(joined(b)));
    if (c->d_ev) (void) hipFree(c->d_ev);
    if (c->h_ev) (void) hipHostFree(c->h_ev);
    if (c->d_list) (void) hipFree(c->d_list);
    if (c->h_list) (void) hipHostFree(c->h_list);
    c->d_ev = nullptr;
    c->h_ev = nullptr;
    c->d_list = nullptr;
    c->h_list = nullptr;
    c->slots_cap = 0;
    SPG_TRY(hipMalloc(&c->d_ev, (size_t) slots*b->c.n_ch*2*sizeof(uint32_t)));
    SPG_TRY(hipHostMalloc(&c->h_ev, (size_t) slots*b->c.n_ch*2*sizeof(uint32_t)));
    SPG_TRY(hipMalloc(&c->d_list, ((size_t) slots*b->c.n_ch*3 + 2)*sizeof(uint32_t)));
    SPG_TRY(hipHostMalloc(&c->h_list, ((size_t) slots*b->c.n_ch*3 + 2)*sizeof(uint32_t)));
    SPG_TRY(hipMemset(c->d_list, 0, 2*sizeof(uint32_t)));
    c->which = 0;
    c->slots_cap = slots;
    return SPANGPU_OK;
}

extern "C" {

// ---- super-tone cadences (src/super_tone_rx.c:164-228, :364-448) on the device ------------------------------------------
int spangpu_bank_set_cadences(spangpu_bank_t *b, const int32_t *tone_elems, int n_tones, const spangpu_cadence_elem_t *elems,
                              int want_segments)
{
    if (b == nullptr  ||  n_tones < 0  ||  (n_tones > 0  &&  (tone_elems == nullptr  ||  elems == nullptr)))
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (b->kind != SPANGPU_SUPER_TONE)
        return failf(SPANGPU_ERR_UNSUPPORTED, "cadences belong to a super-tone bank");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    std::vector<int32_t> first(n_tones + 1, 0);
    for (int t = 0;  t < n_tones;  t++)
    {
        if (tone_elems[t] < 0)
            return failf(SPANGPU_ERR_BAD_ARG, "tone %d has a negative element count", t);
        first[t + 1] = first[t] + tone_elems[t];
    }
    const int n_elems = first[n_tones];
    std::vector<int4> el(n_elems > 0  ?  n_elems  :  1);
    for (int i = 0;  i < n_elems;  i++)
    {
        if (elems[i].f1 < -1  ||  elems[i].f1 >= 255  ||  elems[i].f2 < -1  ||  elems[i].f2 >= 255  ||  elems[i].min_ms < 0
            ||  elems[i].max_ms < 0  ||  elems[i].min_ms > 0x7FFFFFFF/8)
            return failf(SPANGPU_ERR_BAD_ARG, "element %d: bins are -1..254, times are milliseconds >= 0", i);
        // milliseconds are kept in samples, 0 = no upper limit (super_tone_rx.c:157-158); a run of b blocks is 128 b samples
        // long, so the window in blocks is ceil(lo/128) .. floor(hi/128)
        const long long lo = 8LL*elems[i].min_ms;
        const long long hi = (elems[i].max_ms == 0)  ?  0x7FFFFFFFLL  :  8LL*elems[i].max_ms;
        el[i] = make_int4(cad_pair(elems[i].f1, elems[i].f2), (int) ((lo + 127)/128), (int) ((hi > 0x7FFFFFFFLL  ?  0x7FFFFFFFLL  :  hi)/128), 0);
    }
    Cadence *c = b->cad;
    const bool fresh = (c == nullptr);
    if (fresh)
    {
        if ((c = (Cadence *) calloc(1, sizeof(Cadence))) == nullptr)
            return failf(SPANGPU_ERR_NO_MEMORY, "out of memory");
        if (hipMalloc(&c->d_state, (size_t) kCadWords*b->c.n_ch*sizeof(int32_t)) != hipSuccess
            ||  hipMalloc(&c->d_count, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess
            ||  hipHostMalloc(&c->h_count, (size_t) b->c.n_ch*sizeof(int32_t)) != hipSuccess)
        {
            cadence_free(c);
            return failf(SPANGPU_ERR_NO_MEMORY, "out of device memory for the cadence state");
        }
        hipLaunchKernelGGL(cadence_init_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, joined(b), c->d_state, b->c.n_ch, 0, b->c.n_ch);
        c->done_serial = b->launch_serial;      // what was received before now is not matched
        b->cad = c;
        const int rc = cadence_event_room(b, kCadSlotsPerBlock*((b->maxb_cap > 2)  ?  b->maxb_cap  :  2));
        if (rc != SPANGPU_OK)
            return rc;
    }
    // the new tables are made and filled first and swapped in only when they are complete: a failure leaves the bank on
    // its old set (a live bank's next launch reads first[] and elem[] on the device)
    {
        int32_t *n_first = nullptr;
        int4 *n_elem = nullptr;
        if (hipMalloc(&n_first, first.size()*sizeof(int32_t)) != hipSuccess
            ||  hipMalloc(&n_elem, el.size()*sizeof(int4)) != hipSuccess
            ||  hipMemcpy(n_first, first.data(), first.size()*sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess
            ||  hipMemcpy(n_elem, el.data(), el.size()*sizeof(int4), hipMemcpyHostToDevice) != hipSuccess)
        {
            if (n_first) (void) hipFree(n_first);
            if (n_elem) (void) hipFree(n_elem);
            return failf(SPANGPU_ERR_NO_MEMORY, "out of device memory for the cadence tables");
        }
        SPG_TRY(hipStreamSynchronize(joined(b)));        // no launch still reads the old ones
        if (c->d_first) (void) hipFree(c->d_first);
        if (c->d_elem) (void) hipFree(c->d_elem);
        c->d_first = n_first;
        c->d_elem = n_elem;
    }
    if (!fresh)
    {
        // the tone numbers of the old set mean nothing in the new one: nobody is following a tone (the run histories stay)
        // (-2, not -1: "none, and look at every cadence at the next block" -- the channel may be in the middle of a run that
        // one of the new cadences ends with, see cadence_dev.hpp)
        SPG_TRY(hipMemsetD32Async((hipDeviceptr_t) (c->d_state + (size_t) 2*b->c.n_ch), (int) 0xFFFFFFFEu, (size_t) b->c.n_ch, joined(b)));
        SPG_TRY(hipMemsetAsync(c->d_state + (size_t) 3*b->c.n_ch, 0, (size_t) b->c.n_ch*sizeof(int32_t), joined(b)));
    }
    c->n_tones = n_tones;
    c->n_elems = n_elems;
    for (int t = 0;  t < n_tones  &&  t < kCadLdsTones;  t++)
        c->tone_len[t] = first[t + 1] - first[t];
    c->segments = want_segments  ?  1  :  0;
    SPG_TRY(hipStreamSynchronize(joined(b)));
    return SPANGPU_OK;
}

int spangpu_bank_cadence_run(spangpu_bank_t *b)
{
    if (b == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "null bank");
    Cadence *c = b->cad;
    if (c == nullptr)
        return failf(SPANGPU_ERR_STATE, "no cadences were given to this bank (spangpu_bank_set_cadences)");
    if (c->done_serial == b->launch_serial)
        return c->last_slots;
    SPG_TRY(hipSetDevice(b->c.device));
    const int slots = kCadSlotsPerBlock*b->last_maxb;
    if (c->fused)
    {
        // the detector launch did it
        c->fused = false;
        c->done_serial = b->launch_serial;
        c->last_slots = slots;
        return slots;
    }
    const int rc = cadence_event_room(b, slots);
    if (rc != SPANGPU_OK)
        return rc;
    if (b->last_maxb > 0)
    {
        CadenceArgs A;
        c->which ^= 1;
        c->list_due = false;
        cadence_args(b, c, A, c->which);
        hipLaunchKernelGGL(cadence_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, joined(b),
                           (const uint32_t *) records_of(b), b->c.n_ch, b->last_maxb, A);
        SPG_TRY(hipGetLastError());
    }
    else
    {
        SPG_TRY(hipMemsetAsync(c->d_count, 0, (size_t) b->c.n_ch*sizeof(int32_t), joined(b)));
    }
    c->done_serial = b->launch_serial;
    c->last_slots = slots;
    return slots;
}

int spangpu_bank_cadence_events(spangpu_bank_t *b, const uint32_t **events, const int32_t **counts)
{
    const int slots = spangpu_bank_cadence_run(b);
    if (slots < 0)
        return slots;
    Cadence *c = b->cad;
    SPG_TRY(hipMemcpyAsync(c->h_count, c->d_count, (size_t) b->c.n_ch*sizeof(int32_t), hipMemcpyDeviceToHost, joined(b)));
    if (slots > 0)
        SPG_TRY(hipMemcpyAsync(c->h_ev, c->d_ev, (size_t) slots*b->c.n_ch*2*sizeof(uint32_t), hipMemcpyDeviceToHost, joined(b)));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    if (events)
        *events = c->h_ev;
    if (counts)
        *counts = c->h_count;
    return slots;
}

int spangpu_bank_cadence_list(spangpu_bank_t *b, const uint32_t **list)
{
    const int slots = spangpu_bank_cadence_run(b);
    if (slots < 0)
        return slots;
    Cadence *c = b->cad;
    if (slots == 0  ||  c->d_list == nullptr  ||  b->last_maxb <= 0)
        return 0;
    if (c->list_due)
    {
        CadenceArgs A;
        c->which ^= 1;
        c->list_due = false;
        cadence_args(b, c, A, c->which);
        hipLaunchKernelGGL(cadence_list_kernel, dim3((b->c.n_ch + 255)/256), dim3(256), 0, joined(b), b->c.n_ch, A);
        SPG_TRY(hipGetLastError());
    }
    // as a rule a tick has few reports: one small copy brings the counters and the first of them
    const size_t cap = (size_t) c->slots_cap*b->c.n_ch;
    const size_t first = (cap < 4096)  ?  cap  :  4096;
    SPG_TRY(hipMemcpyAsync(c->h_list, c->d_list, (2 + 3*first)*sizeof(uint32_t), hipMemcpyDeviceToHost, joined(b)));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    const size_t n = c->h_list[c->which];
    if (n > cap)
        return failf(SPANGPU_ERR_STATE, "cadence event list overran its buffer");
    if (n > first)
    {
        SPG_TRY(hipMemcpyAsync(c->h_list + 2 + 3*first, c->d_list + 2 + 3*first, 3*(n - first)*sizeof(uint32_t), hipMemcpyDeviceToHost, joined(b)));
        SPG_TRY(hipStreamSynchronize(joined(b)));
    }
    if (list)
        *list = c->h_list + 2;
    return (int) n;
}

int spangpu_bank_cadence_device(spangpu_bank_t *b, const uint32_t **events_dev, const int32_t **counts_dev)
{
    if (b == nullptr  ||  b->cad == nullptr)
        return failf(SPANGPU_ERR_STATE, "no cadences were given to this bank");
    if (events_dev)
        *events_dev = b->cad->d_ev;
    if (counts_dev)
        *counts_dev = b->cad->d_count;
    return b->cad->last_slots;
}

int spangpu_bank_cadence_reset(spangpu_bank_t *b, int channel)
{
    if (b == nullptr  ||  b->cad == nullptr)
        return failf(SPANGPU_ERR_STATE, "no cadences were given to this bank");
    if (channel < -1  ||  channel >= b->c.n_ch)
        return failf(SPANGPU_ERR_BAD_ARG, "bad channel");
    SPG_TRY(hipSetDevice(b->c.device));
    const int first = (channel < 0)  ?  0  :  channel;
    const int n = (channel < 0)  ?  b->c.n_ch  :  1;
    hipLaunchKernelGGL(cadence_init_kernel, dim3((n + 255)/256), dim3(256), 0, joined(b), b->cad->d_state, b->c.n_ch, first, n);
    SPG_TRY(hipGetLastError());
    return SPANGPU_OK;
}

int spangpu_bank_cadence_state_words(void)
{
    return kCadWords;
}

int spangpu_bank_cadence_get_state(spangpu_bank_t *b, int channel, int32_t *words)
{
    if (b == nullptr  ||  b->cad == nullptr)
        return failf(SPANGPU_ERR_STATE, "no cadences were given to this bank");
    if (channel < 0  ||  channel >= b->c.n_ch  ||  words == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    SPG_TRY(hipMemcpy2D(words, sizeof(int32_t), b->cad->d_state + channel, (size_t) b->c.n_ch*sizeof(int32_t), sizeof(int32_t), kCadWords,
                        hipMemcpyDeviceToHost));
    if (words[2] < -1)
        words[2] = -1;          // -2 is the engine's own "none, and every cadence is looked at once at the next block" (cadence_dev.hpp)
    return kCadWords;
}

int spangpu_bank_cadence_set_state(spangpu_bank_t *b, int channel, const int32_t *words)
{
    if (b == nullptr  ||  b->cad == nullptr)
        return failf(SPANGPU_ERR_STATE, "no cadences were given to this bank");
    if (channel < 0  ||  channel >= b->c.n_ch  ||  words == nullptr)
        return failf(SPANGPU_ERR_BAD_ARG, "bad arguments");
    if (words[2] < -1  ||  words[2] >= b->cad->n_tones  ||  words[3] < 0  ||  words[3] > 255)
        return failf(SPANGPU_ERR_BAD_ARG, "state words out of range");
    SPG_TRY(hipSetDevice(b->c.device));
    SPG_TRY(hipStreamSynchronize(joined(b)));
    int32_t w[kCadWords];
    memcpy(w, words, sizeof(w));
    if (w[2] == -1)
        w[2] = -2;              // a state from outside may sit in the middle of a run a cadence ends with: look at all of them once
    // the elements of the followed cadence that have gone by are counted modulo its length on the device (head of the ring: 0)
    if (w[2] >= 0  &&  w[2] < kCadLdsTones  &&  b->cad->tone_len[w[2]] > 0)
        w[3] = w[3]%b->cad->tone_len[w[2]];
    SPG_TRY(hipMemcpy2D(b->cad->d_state + channel, (size_t) b->c.n_ch*sizeof(int32_t), w, sizeof(int32_t), sizeof(int32_t), kCadWords,
                        hipMemcpyHostToDevice));
    return SPANGPU_OK;
}

}   // extern "C"
