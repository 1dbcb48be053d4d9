// capi_internal.hpp -- entry points one unit of the library offers to the others (csdr__*: exported for tests and
// tools, not in the public header).  The defining and the using units both include this, so a signature that changes
// on one side only does not compile.
#pragma once
#include "../../include/cutesdr_mi.h"

namespace csdr {
struct DcBlank;                                         // downconv_kernels.h
// the last blanked call of a chain batch (csdr__demod_batch_last_blank): which input it consumed
enum { BLANK_CALL_NONE = 0, BLANK_CALL_ROWS = 1, BLANK_CALL_PACKETS = 2 };
struct BlankCall {
    int form;                                           // BLANK_CALL_*
    const void *src;                                    // d_in / d_packets
    long long stride;                                   // rows: in_stride; datagrams: pkt_len
    int n;                                              // samples per channel
};
// what a plotter batch reads of a spectrum batch at a draw (csdr__fft_batch_view)
struct FftView {
    int device, channels, size, invert;                 // as they are at the call
    double fs;
    const float *d_ave;                                 // [channels][size] bels, display order
    const int *d_over;                                  // [channels] overload words of the last put
};
}

extern "C" {
/* capi_downconv.hip */
int csdr__downconvert_batch_process_rows(csdr_downconvert_batch *b, const float *d_in, long long in_stride,
                                         const int *d_in_rows, int n_per_channel, float *d_out, long long out_stride,
                                         void *stream, const void *d_packets, int pkt_len, const csdr::DcBlank *blank);
int csdr__downconvert_batch_set_wgs(csdr_downconvert_batch *b, long wgs);
int csdr__downconvert_batch_copy_channel(csdr_downconvert_batch *dst, int dc, csdr_downconvert_batch *src, int sc);
/* capi_fastfir.hip */
int csdr__fastfir_batch_copy_row(csdr_fastfir_batch *dst, int dr, csdr_fastfir_batch *src, int sr);
/* capi_frontend.hip */
int csdr__noiseproc_batch_mask(csdr_noiseproc_batch *b, const float *d_in, long long in_stride, const void *d_packets,
                               int npackets, int pkt_len, int n_per_channel, unsigned *d_mask, long long mask_stride,
                               const void **d_state, const float **d_hist, void *stream);
int csdr__noiseproc_batch_shape(csdr_noiseproc_batch *b, int *channels, int *device);
int csdr__noiseproc_batch_process_packets(csdr_noiseproc_batch *b, const void *d_packets, int npackets, int pkt_len,
                                          float *d_out, long long out_stride, void *stream);
/* capi_fft.hip */
int csdr__fft_batch_view(csdr_fft_batch *f, csdr::FftView *v);
/* capi_demod_batch.hip */
int csdr__demod_batch_wait_input_free(csdr_demod_batch *b, void *stream);
int csdr__demod_batch_last_blank(csdr_demod_batch *b, csdr::DcBlank *blank, csdr::BlankCall *call, int *channels, int *device);
int csdr__demod_batch_blank_for(csdr_demod_batch *b, const char *what, int channels, int device, int form, const void *src,
                                long long stride, int n, csdr::DcBlank *blank);
}
