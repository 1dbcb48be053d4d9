// What the reference's dsp/ files expect from the rest of the application: the test bench object their PROFILE_* calls
// go to (here the recording stub) and the six timing hooks of interface/perform.h, which do nothing.
#include "gui/testbench.h"
#include "interface/perform.h"
static CTestBench s_bench;
CTestBench *g_pTestBench = &s_bench;
void InitPerformance() {}
void StartPerformance() {}
void StopPerformance(int) {}
void ReadPerformance() {}
void SamplePerformance() {}
int GetDeltaPerformance() { return 0; }
