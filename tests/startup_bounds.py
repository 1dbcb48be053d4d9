"""Start-up tolerances of the END-TO-END chain comparisons, derived -- not fitted (VERDICT r5 task 4).

Where an fp32 chain cannot follow the fp64 one word for word is the start of a stream: the band-pass filter's output
starts at 1e-12 of full scale (its pre-ringing), the AGC behind it is at full gain (x 7e4 below the knee), and an fp32
FFT filter hands over its own rounding there -- samples that are small multiples of one quantum (2^-15 for a carrier of
3277: tools/experiments/r6_sam_zero_probe.py), 3...5e-7 of the largest input in absolute terms (K1's measured error).
A PLL behind the AGC takes the PHASE of those samples.  How far that moves the audio is a property of the REFERENCE's
arithmetic, measured on the oracle alone: tests/test_oracle_independent.py::test_startup_spread_* runs the oracle chain
twice -- on its own fp64 filter output, and with that output disturbed like an fp32 filter's (additive noise of 3e-7 of
the largest filter input; the same floor as a grid of 1e-8) -- and records the per-burst spread between the two runs
over several seeds.  The numbers below are those spreads (maximum over seeds and disturbances, rounded up); the GPU
bounds are SPREAD x FACTOR.  The CPU test fails when the oracle stops reproducing a spread (within x 1/3 ... x 1.5), so
a bound cannot drift away from what justifies it.

What the derivation found (round 6):
  * relative fp32 rounding of the filter output (1 ulp per sample) moves NOTHING (1e-8 of full scale): it is the
    ABSOLUTE floor of the fp32 FFT that matters, during the start-up only;
  * FM: the burst of the pull-in is arbitrary (0.8 ... 1.6 of full scale), then the difference decays x 5 per burst
    (x 3.7 behind a 10 MSPS chain's shorter bursts in time);
  * SAM stereo is BISTABLE in its first two bursts: about half of the seeds drive the 100 Hz loop's integrator into its
    limit while the filter still starts up, and the two outcomes differ by 0.48 / 1.70 of full scale (both channels carry
    the quadrature component); from the third burst 5e-6.  SAM mono (the in-phase component only): 1.3e-3 / 2.6e-4;
  * AM / SSB / CW: 3e-4 in the first burst (AGC at full gain on the floor), nothing behind it.
The stages behind the filter are pinned WITHOUT any start-up allowance by
tests/test_chain_taps_gpu.py::test_post_chain_on_the_gpus_own_filter_output_from_the_first_sample.

Behind the 16384-point filter a burst is 8192 samples, and the stream's first burst holds eight times as much start-up:
the whole pull-in of every loop and the AGC's whole descent from full gain.  The same measurement there
(_startup_spread(oracle, mode, stereo, 2e6, 16384, 80), six seeds; CW 160 windows): everything is in burst 0, behind it
at most 6.1e-7 (on the batch tests' tones 1.2e-6; FM 3.9e-6 mono / 5.5e-6 stereo in burst 1, then 1.2e-7) -- at least
five times below the steady bounds, which therefore hold from the second burst on.  Two inputs are recorded: the one the
single-chain tests use (test_chain_parity_gpu.chain_input), and the rows of the batch rig
(test_batch_control_combinations_gpu._signal at -20 dBFS), whose SSB / CW input is six tones and gives three times the
spread; AM, SAM and FM measure the same on both.  A test takes the list of the input it runs on."""
FACTOR = 2.0

# per-burst spread of the oracle chain, in units of full scale (32767); index = bursts behind the burst of the pull-in
FM_SPREAD = [None, 2.8e-2, 4.9e-3, 1.0e-3, 1.9e-4, 3.7e-5]               # the 2 MSPS chain's (the 10 MSPS chain stays below it)
SAM_MONO_SPREAD = [1.4e-3, 2.7e-4]                                       # bursts 0 and 1 of the stream
SAM_STEREO_SPREAD = [0.49, 1.70, 5.2e-6]                                  # bursts 0, 1 (bistable) and 2
LINEAR_SPREAD = [3.0e-4]                                                  # AM / SSB / CW, burst 0

FM_STARTUP = [None] + [FACTOR * s for s in FM_SPREAD[1:]]                 # bound k bursts behind the pull-in; None = arbitrary
SAM_FIRST, SAM_SECOND = FACTOR * SAM_MONO_SPREAD[0], FACTOR * SAM_MONO_SPREAD[1]
SAM_STEREO_BISTABLE = 2.5                                                 # bursts 0 and 1: within the audio range, no more can be asked

# ---- 16384-point filter, bursts of 8192 samples: the spread of burst 0 (mono unless named), full scale
SPREAD_16K = {"AM": 3.5e-3, "USB": 4.2e-3, "LSB": 4.1e-3, "CWU": 4.7e-3, "SAM": 9.5e-3}            # chain_input
SPREAD_16K_STEREO = {"AM": 5.0e-3, "SAM": 1.70}                                                  # SAM stereo: bistable, as at 2048
SPREAD_16K_RIG = {"AM": 3.5e-3, "USB": 1.2e-2, "LSB": 1.2e-2, "CWU": 1.4e-2, "SAM": 9.5e-3}        # the batch rig's rows (_signal)
FM_SPREAD_16K = [1.57, 3.9e-6]                  # burst 0 is the pull-in (arbitrary), burst 1; stereo 2.2 / 5.5e-6
FM_SPREAD_16K_STEREO = [2.2, 5.5e-6]
LATER_16K, LATER_16K_RIG = 6.1e-7, 1.2e-6       # every mode but FM, every burst behind the first


def first_burst_16k(mode, stereo, rig):
    """GPU bound of the first 8192-sample burst of a stream, in units of full scale; None: arbitrary (FM's pull-in)"""
    if mode == "FM":
        return None
    if mode == "SAM" and stereo:
        return SAM_STEREO_BISTABLE
    if stereo:
        return FACTOR * SPREAD_16K_STEREO[mode]
    return FACTOR * (SPREAD_16K_RIG if rig else SPREAD_16K)[mode]
