// gui/testbench.h as the reference build sees it: the recording stub of tests/cpp/stub/gui/testbench.h plus the three
// profile numbers that only the reference's own dsp/ files name (noiseproc.cpp uses PROFILE_7).
#ifndef CSDR_REF_TESTBENCH_H
#define CSDR_REF_TESTBENCH_H
#include "../../../tests/cpp/stub/gui/testbench.h"
#define PROFILE_5 5
#define PROFILE_6 6
#define PROFILE_7 7
#endif
