"""A batch estimator on the oracle for replay.run_sessions (tests only): what estimate_poses does in one multi-map
launch, one OracleEstimator at a time, with the number of calls kept."""


class OracleBatchEstimate:
    def __init__(self):
        self.calls = []                 # batch size of every call

    def __call__(self, estims, initPoses):
        estims = list(estims)
        self.calls.append(len(estims))
        return [e.estimatePose(p) for e, p in zip(estims, initPoses)]
