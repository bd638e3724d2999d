"""GE2E speaker encoder of DiffVC (DiffVC/speaker_encoder/encoder) with the network on the HIP kernels of csrc/spk.hip.

Same module names, function names, signatures and state_dict keys as the reference package, importable with torch and numpy alone:
`inference` (load_model, embed_utterance, ...), `audio` (preprocessing, power mel), `model` (SpeakerEncoder), `params_data`,
`params_model`.  GE2E training (similarity matrix, loss) is not part of it."""
