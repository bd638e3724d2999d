"""DiffVC on MI355X: `model` mirrors DiffVC/model (decoder, MelEncoder, PostNet, the DiffVC / FwdDiffusion shells) and
`speaker_encoder/encoder` mirrors DiffVC/speaker_encoder/encoder (the GE2E network that produces the speaker embedding `c`,
csrc/spk.hip), each with the reference's names, signatures and state_dict keys."""
