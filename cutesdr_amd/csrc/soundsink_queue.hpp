// soundsink_queue.hpp -- the host half of CSoundOut (reference interface/soundout.cpp:155-468) shared by the single
// sink (capi_soundsink.hip) and the batch sink (capi_soundsink_batch.hip): the 16384-entry output queue, the fill
// average and the P-controller CalcError.  No locking here: every caller holds the mutex of the sink (or of the
// batch's receiver) that owns the queue.  Blocking mode belongs to the single sink alone and stays in its file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace csdr {
namespace sinkq {
constexpr int kQ = 16384;                 // OUTQSIZE (soundout.h:18)
constexpr int kRate = 48000;              // SOUNDCARD_RATE (soundout.cpp:48)
constexpr double kAlpha = 0.001;          // FILTERQLEVEL_ALPHA (:51)
constexpr double kPGain = 2.38e-7;        // P_GAIN (:52)
constexpr int kMaxIn = 8192;              // the resampler's MaxInputSize (:71)
}

struct SinkQueue {
    int stereo = 0;
    bool startup = true;                  // m_Startup
    double user_rate = sinkq::kRate, out_ratio = 1.0, rate_corr = 0.0, gain = 1.0, ave_level = 0.0;
    int head = 0, tail = 0, level = 0, rate_count = 0, ppm = 0;
    std::vector<short> q;                 // the ring (2 shorts per entry when stereo)

    void init(int st)
    {
        stereo = st != 0;
        q.assign((size_t)(stereo ? 2 : 1) * sinkq::kQ, 0);
    }
    // ChangeUserDataRate (:155-175): clears the queue only; the resampler keeps its state
    void change_user_data_rate(double rate)
    {
        if (user_rate != rate) {
            user_rate = rate;
            std::fill(q.begin(), q.end(), (short)0);
            out_ratio = rate / (double)sinkq::kRate;
            head = tail = level = 0;
            ave_level = sinkq::kQ / 2;
            startup = true;
        }
    }
    // SetVolume (:180-189): 0 mutes, 1..99 = -50 dB .. 0 dB
    void set_volume(int vol)
    {
        if (vol == 0) gain = 0.0;
        else if (vol <= 99) gain = std::pow(10.0, ((double)vol - 99.0) / 39.2);
    }
    double rate() const { return 1.0 * out_ratio * (1.0 + rate_corr); }   // TEST_ERROR * m_OutRatio * (1 + m_RateCorrection)
    bool full_next() const { return ((head + 1) & (sinkq::kQ - 1)) == tail; }
    // one resampled entry r[i] at the head
    void store(const short *r, int i)
    {
        if (stereo) { q[2 * head] = r[2 * i]; q[2 * head + 1] = r[2 * i + 1]; }
        else q[head] = r[i];
        head = (head + 1) & (sinkq::kQ - 1);
        level++;
    }
    // PutOutQueue's non-blocking branch (:221-247 / :279-305) for entries i..k-1 of r, then the fill average
    void push(const short *r, int i, int k)
    {
        bool overflow = false;
        for (; i < k; i++) {
            store(r, i);
            if (head == tail) {                             // full: drop a quarter of the queue (:228-236)
                tail = (tail + sinkq::kQ / 4) & (sinkq::kQ - 1);
                level -= sinkq::kQ / 4;
                overflow = true;
                break;
            }
        }
        if (overflow) ave_level = level;
        ave_level = (1.0 - sinkq::kAlpha) * ave_level + sinkq::kAlpha * (double)level;
    }
    // GetOutQueue's start-up (:316-333): true while the sink is still silent (out is zeroed then)
    bool silent(int n, short *out)
    {
        if (!startup) return false;
        const int w = stereo ? 2 : 1;
        std::memset(out, 0, sizeof(short) * (size_t)w * n);
        if (level > sinkq::kQ / 2) {
            startup = false;
            rate_count = -5 * sinkq::kRate;                 // first update delayed to let the level settle
            ppm = 0;
            ave_level = level;
            return false;
        }
        return true;
    }
    // GetOutQueue's pop loop (:334-353); returns whether it ran empty
    bool pop(int n, short *out)
    {
        bool underflow = false;
        for (int i = 0; i < n; i++) {
            if (head != tail) {
                if (stereo) { out[2 * i] = q[2 * tail]; out[2 * i + 1] = q[2 * tail + 1]; }
                else out[i] = q[tail];
                tail = (tail + 1) & (sinkq::kQ - 1);
                level--;
            } else {                                        // empty: back up a quarter and repeat older data (:344-351)
                tail = (tail - sinkq::kQ / 4) & (sinkq::kQ - 1);
                if (stereo) { out[2 * i] = q[2 * tail]; out[2 * i + 1] = q[2 * tail + 1]; }
                else out[i] = q[tail];
                level += sinkq::kQ / 4;
                underflow = true;
            }
        }
        return underflow;
    }
    // the fill average after a get and CalcError (:456-468), every second of consumed samples
    void rate_loop(int n, bool underflow)
    {
        ave_level = (1.0 - sinkq::kAlpha) * ave_level + sinkq::kAlpha * level;
        if (underflow) ave_level = level;
        rate_count += n;
        if (rate_count >= sinkq::kRate) {
            rate_corr = (double)(ave_level - sinkq::kQ / 2) * sinkq::kPGain;
            ppm = (int)(rate_corr * 1e6);
            rate_count = 0;
        }
    }
    // the whole non-blocking GetOutQueue (:311-375 mono, :381-445 stereo)
    void get(int n, short *out)
    {
        if (silent(n, out)) return;
        rate_loop(n, pop(n, out));
    }
};

}  // namespace csdr
