"""Drop-in for DiffVC/speaker_encoder: put this directory on sys.path and `from encoder import inference as spk_encoder`."""
