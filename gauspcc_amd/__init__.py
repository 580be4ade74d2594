"""gauspcc_amd -- the GausPcgc hot path of Wangkkklll/GausPcc on MI355X.

Importing the package has no side effects on the host application: no environment variable is touched, no GPU call is made.
A process that keeps more than one codec context busy on a GPU (two scenes in flight, `--jobs 2`) gets as much overlap
between them as the hardware queues the HIP runtime gives the process allow: a context of this library uses three streams,
and contexts whose streams share queues run in lockstep (HISTORY.md section 7).  The queue count is the environment's to set."""
