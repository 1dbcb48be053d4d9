"""The NCO-spur bookkeeping of CSdrInterface (reference interface/sdrinterface.cpp:791-824 ManageNCOSpurOffsets,
:829-848 NcoSpurCalibrate, :886-887 its caller) restated as a plain per-call loop -- the yardstick of the spur
calibration tests.  The arithmetic of :833-840 is not restated: `calibrate` is handed in (the fp64 checker's own
function in the GPU tests, nothing in the bookkeeping tests).

    ManageNCOSpurOffsets(cmd, pI, pQ):                               NcoSpurCalibrate(pData, length):
        m_NcoSpurCalActive = FALSE;                          :793        if (m_NcoSpurCalCount < SPUR_CAL_MAXSAMPLES) {   :831
        SET:      I = *pI; Q = *pQ;                          :799-800        ... the recurrence over length doubles ...   :833-840
        STARTCAL: if (I > 10.0 || I < -10.0) I = 0.0;        :805-806        m_NcoSpurCalCount += (length / 4);           :841
                  if (Q > 10.0 || Q < -10.0) Q = 0.0;        :807-808    } else
                  m_NcoSpurCalCount = 0; Active = TRUE;      :809-810        m_NcoSpurCalActive = FALSE;                  :845
        READ:     *pI = I; *pQ = Q;                          :816-817
    ProcessIQData: if (m_NcoSpurCalActive) NcoSpurCalibrate(pIQData, Length);                                            :886-887
"""
SPUR_CAL_MAXSAMPLES = 300000             # sdrinterface.cpp:47


class RefSpurCal:
    def __init__(self, calibrate=None):
        self.off = [0.0, 0.0]            # m_NCOSpurOffsetI, m_NCOSpurOffsetQ
        self.count = 0                   # m_NcoSpurCalCount
        self.active = False              # m_NcoSpurCalActive
        self.calibrate = calibrate       # (off, samples) -> off: the recurrence of :833-840
        self.ran = 0                     # calls in which the recurrence ran

    def set(self, i, q):
        self.active = False              # :793
        self.off = [float(i), float(q)]  # :799-800

    def start_cal(self):
        self.active = False              # :793
        if self.off[0] > 10.0 or self.off[0] < -10.0:   # :805-806
            self.off[0] = 0.0
        if self.off[1] > 10.0 or self.off[1] < -10.0:   # :807-808
            self.off[1] = 0.0
        self.count = 0                   # :809
        self.active = True               # :810

    def read(self):
        self.active = False              # :793
        return tuple(self.off)           # :816-817

    def call(self, nsamples, samples=None):
        """one ProcessIQData call of nsamples complex samples (Length = 2 * nsamples doubles)"""
        if not self.active:              # :886
            return
        if self.count < SPUR_CAL_MAXSAMPLES:            # :831
            if self.calibrate is not None:
                self.off = [float(v) for v in self.calibrate(self.off, samples)]
            self.ran += 1
            self.count += (2 * nsamples) // 4           # :841
        else:
            self.active = False          # :845

    def state(self):
        return self.off[0], self.off[1], self.count, self.active
